"""The host-side handling of regression data blocks (smcnuts_amd/csrc/smcn_regdata.hpp: reg_check, reg_repack, reg_splice)
against outputs recorded from the per-model routines it replaced, under the address and undefined-behaviour sanitizers.

tests/regdata_driver.cpp (a stand-alone program that includes only the header) is compiled with
`g++ -fsanitize=address,undefined -fno-sanitize-recover=all`, run once over the cases `cases()` builds from fixed seeds,
and every field it prints -- the check message byte for byte, the layout's integers, the repacked image and the spliced
block bit for bit -- is compared with tests/golden/regdata_parent.npz.  Every block is a heap array of exactly its length,
so a read past a caller-supplied length fails the run.

How the fixture was recorded.  At the commit before the header existed, the four per-model block checks, the routine
that repacked a model's table and the header-check and splice lines of `smcn_predict_set_data` were lifted verbatim
from smcn_api.hip (the layout helpers from smcn_models.hpp) into a scratch file named smcn_regdata.hpp that wraps them
in the three function signatures (the layout's integers written down from the expressions those routines index with);
this driver was compiled against that file in place of the real header and `python tests/test_regdata_host.py
<that driver> tests/golden/regdata_parent.npz` stored what it printed.  The fixture therefore comes from the old
routines, not from the code under test, and is not re-recorded when this header changes.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "regdata_parent.npz")
GLM, HGLM, CAT, ORD = 4, 5, 6, 7
NAN, INF = float("nan"), float("inf")
# distinct non-empty messages the four replaced checks could return (17 GLM + 17 hierarchical + 10 categorical + 8 ordinal)
N_CHECK_MESSAGES = 52


# ---- blocks -----------------------------------------------------------------------------------------------------------
def _grid(rng, k):
    """k values on a grid of eighths in [-2, 2]: exact in binary, and few distinct bit patterns (a small fixture)"""
    return (rng.integers(-16, 17, size=k) / 8.0).tolist()


def _sds(rng, k):
    return rng.choice([0.5, 1.0, 2.0, 2.5], size=k).tolist()


def _y(rng, fam, n):
    if fam == 0:
        return rng.integers(0, 2, size=n).astype(float).tolist()
    if fam == 2:
        return _grid(rng, n)
    return rng.integers(0, 7, size=n).astype(float).tolist()


def block(rng, model, s0, n, p, ic=0, J=0, priors=True):
    """A valid data block (priors=False: the new rows' block of smcn_predict_set_data, without them)."""
    Dc = p + ic
    if model == GLM:
        head, pri = [s0, n, p, ic], _sds(rng, Dc) + ([_grid(rng, 1)[0], 1.5] if s0 >= 2 else [])
        body = _y(rng, s0, n)
    elif model == HGLM:
        head, pri = [s0, n, p, ic, J], _sds(rng, Dc) + [0.75] + ([_grid(rng, 1)[0], 1.5] if s0 >= 2 else [])
        body = _y(rng, s0, n) + rng.integers(0, J, size=n).astype(float).tolist()
    elif model == CAT:
        head, pri = [s0, n, p, ic], _sds(rng, (s0 - 1) * Dc)
        body = rng.integers(0, s0, size=n).astype(float).tolist()
    else:
        head, pri = [s0, n, p], _sds(rng, p + s0 - 1)
        body = rng.integers(0, s0, size=n).astype(float).tolist()
    return [float(v) for v in head + (pri if priors else []) + body + _grid(rng, n * p)]


def _variants():
    """(model, first header slot, J) of every model variant the valid grid covers"""
    v = [(GLM, f, 0) for f in range(4)] + [(HGLM, f, J) for f in range(4) for J in (1, 3)]
    return v + [(CAT, K, 0) for K in (2, 3, 16)] + [(ORD, K, 0) for K in (2, 5)]


def _with(b, i, v):
    b = list(b)
    b[i] = v
    return b


def cases():
    """[(name, model, block, new rows' block or None)]"""
    out = []
    rng = np.random.default_rng(20261018)
    # valid: every variant at every n (either side of the 64-row padding) with p and the intercept rotating, so that each
    # variant sees every p, both intercept settings and both parities of the row's column count.  n, p and the intercept
    # are rotated, not crossed: the full product is 544 images of up to 1 400 doubles, several hundred KB of fixture, and
    # n (padding), p and the intercept (row width, columns) act on the image independently of one another
    ns, ps = (1, 63, 64, 65), (0, 1, 2, 5)
    for k, (model, s0, J) in enumerate(_variants()):
        for i, n in enumerate(ns):
            p, ic = ps[(k + i) % 4], (k + i // 2) % 2
            if model == ORD:
                ic = 0
            elif p == 0:
                ic = 1                                  # (p = 0 without an intercept is refused)
            if model == CAT and s0 == 16 and p == 5:
                p = 3                                   # (K - 1) Dc <= 64
            out.append((f"ok-m{model}-s{s0}-J{J}-n{n}-p{p}-ic{ic}", model, block(rng, model, s0, n, p, ic, J), None))
    out.append(("ok-ord-p0-K5", ORD, block(rng, ORD, 5, 65, 0), None))
    out.append(("ok-ord-p0-K2", ORD, block(rng, ORD, 2, 1, 0), None))

    # D = 64 accepted, D = 65 refused (the refusal comes before the length check: a header is enough)
    for name, model, s0, p, ic, J in (("glm", GLM, 1, 63, 1, 0), ("glmdisp", GLM, 3, 62, 1, 0), ("hglm", HGLM, 0, 59, 1, 3),
                                      ("hglmdisp", HGLM, 2, 58, 1, 3), ("cat", CAT, 2, 63, 1, 0), ("ord", ORD, 5, 60, 0, 0),
                                      ("ordK65", ORD, 65, 0, 0, 0)):
        b = block(rng, model, s0, 1, p, ic, J)
        out.append((f"D64-{name}", model, b, None))
        wide = _with(b, 0, 66.0) if name == "ordK65" else _with(b, 2, p + 1)
        out.append((f"D65-{name}", model, wide, None))

    # invalid: from one small valid block per model variant
    base = {"glm": (GLM, block(rng, GLM, 1, 3, 2, 1)), "glm0": (GLM, block(rng, GLM, 0, 3, 2, 1)),
            "glm2": (GLM, block(rng, GLM, 2, 3, 2, 1)), "glm3": (GLM, block(rng, GLM, 3, 3, 2, 1)),
            "hglm": (HGLM, block(rng, HGLM, 1, 3, 2, 1, 2)), "hglm0": (HGLM, block(rng, HGLM, 0, 3, 2, 1, 2)),
            "hglm2": (HGLM, block(rng, HGLM, 2, 3, 2, 1, 2)), "hglm3": (HGLM, block(rng, HGLM, 3, 3, 2, 1, 2)),
            "cat": (CAT, block(rng, CAT, 3, 3, 2, 1)), "ord": (ORD, block(rng, ORD, 3, 3, 2))}

    def bad(tag, key, b):
        out.append((f"bad-{key}-{tag}", base[key][0], [float(v) for v in b], None))

    for key, (model, b) in base.items():
        nh = {GLM: 4, HGLM: 5, CAT: 4, ORD: 3}[model]
        for q in range(nh):
            bad(f"nan-slot{q}", key, _with(b, q, NAN))
        bad("len-short", key, b[:-1])
        bad("len-long", key, b + [0.0])
        bad("len-header", key, b[:nh - 1])
        bad("len-one", key, b[:1])
        bad("header-only", key, b[:nh])
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 2147483648.0), ("neg", -1.0), ("inf", INF)):
            bad(f"n-{tag}", key, _with(b, 1, v))
        for tag, v in (("neg", -1.0), ("frac", 0.5), ("big", 1048577.0), ("inf", INF), ("huge", 1e300)):
            bad(f"p-{tag}", key, _with(b, 2, v))
        for tag, v in (("zero", 0.0), ("neg", -1.0), ("inf", INF), ("nan", NAN)):
            bad(f"sd-first-{tag}", key, _with(b, nh, v))
        bad("X-nan", key, _with(b, len(b) - 1, NAN))
        bad("X-inf", key, _with(b, len(b) - 4, -INF))
        if model != ORD:
            for tag, v in (("two", 2.0), ("half", 0.5), ("neg", -1.0)):
                bad(f"ic-{tag}", key, _with(b, 3, v))
            if model != HGLM:
                bad("no-cols", key, _with(_with(b, 2, 0.0), 3, 0.0))
        if model in (GLM, HGLM):
            for tag, v in (("four", 4.0), ("half", 0.5), ("neg", -1.0)):
                bad(f"fam-{tag}", key, _with(b, 0, v))
        else:
            for tag, v in (("one", 1.0), ("frac", 2.5), ("seventeen", 17.0), ("inf", INF), ("zero", 0.0)):
                bad(f"K-{tag}", key, _with(b, 0, v))
    # the priors behind the sds, y, g
    Dc = 3
    bad("sd-last-zero", "glm", _with(base["glm"][1], 4 + Dc - 1, 0.0))
    for key in ("glm2", "glm3"):
        b = base[key][1]
        bad("m_tau-nan", key, _with(b, 4 + Dc, NAN))
        bad("m_tau-inf", key, _with(b, 4 + Dc, INF))
        bad("s_tau-zero", key, _with(b, 5 + Dc, 0.0))
        bad("s_tau-inf", key, _with(b, 5 + Dc, INF))
        bad("laid-out-for-0-1", key, b[:4 + Dc] + b[6 + Dc:])       # a block without m_tau, s_tau naming a dispersion family
        bad("len-two-long", key, b + [0.0, 0.0])
    bad("as-family-2", "glm", _with(base["glm"][1], 0, 2.0))          # the same hint, from a family 1 block renamed
    for key in ("hglm", "hglm0", "hglm2", "hglm3"):
        b = base[key][1]
        bad("s_tau-zero", key, _with(b, 5 + Dc, 0.0))
        bad("s_tau-nan", key, _with(b, 5 + Dc, NAN))
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 1048577.0), ("inf", INF)):
            bad(f"J-{tag}", key, _with(b, 4, v))
        g0 = len(b) - 6 - 3
        for tag, v in (("neg", -1.0), ("J", 2.0), ("frac", 0.5), ("nan", NAN)):
            bad(f"g-{tag}", key, _with(b, g0 + 1, v))
    for key in ("hglm2", "hglm3"):
        b = base[key][1]
        bad("m_d-nan", key, _with(b, 6 + Dc, NAN))
        bad("s_d-zero", key, _with(b, 7 + Dc, 0.0))
        bad("s_d-inf", key, _with(b, 7 + Dc, INF))
    for key in base:
        model, b = base[key]
        y0 = len(b) - 6 - (6 if model == HGLM else 3)
        fam = b[0] if model in (GLM, HGLM) else -1
        ys = {0.0: (2.0, 0.5, -1.0, NAN), 1.0: (-1.0, 0.5, INF, NAN, 2.0 ** 54), 2.0: (INF, -INF, NAN),
              3.0: (-1.0, 0.5, 2.0 ** 54, NAN), -1: (-1.0, 3.0, 0.5, NAN)}[fam]
        for j, v in enumerate(ys):
            bad(f"y-{j}", key, _with(b, y0 + j % 3, v))
        if fam == 3.0:
            bad("y-2^53", key, _with(b, y0, 2.0 ** 53))               # (accepted: the bound is inclusive)

    # splice: 65 new rows accepted; another p; a bad new row; a block shorter than its header
    for key, (model, s0, J) in {"glm": (GLM, 1, 0), "glm3": (GLM, 3, 0), "hglm": (HGLM, 2, 3), "cat": (CAT, 3, 0),
                                "ord": (ORD, 4, 0)}.items():
        ic = 0 if model == ORD else 1
        train = block(rng, model, s0, 3, 2, ic, J)
        rows = block(rng, model, s0, 65, 2, ic, J, priors=False)
        nh = {GLM: 4, HGLM: 5, CAT: 4, ORD: 3}[model]
        out.append((f"splice-ok-{key}", model, train, rows))
        out.append((f"splice-p-differs-{key}", model, train, block(rng, model, s0, 65, 3, ic, J, priors=False)))
        out.append((f"splice-X-inf-{key}", model, train, _with(rows, len(rows) - 7, INF)))
        out.append((f"splice-y-range-{key}", model, train, _with(rows, nh + 64, {GLM: 0.5, HGLM: INF}.get(model, -1.0))))
        out.append((f"splice-short-{key}", model, train, rows[:nh - 1]))
        out.append((f"splice-len-short-{key}", model, train, rows[:-1]))
        if model == HGLM:
            out.append((f"splice-g-range-{key}", model, train, _with(rows, nh + 65 + 64, 3.0)))
            out.append((f"splice-J-differs-{key}", model, train, _with(rows, 4, 4.0)))
    return out


# ---- driver -----------------------------------------------------------------------------------------------------------
def write_cases(path, cs):
    with open(path, "w") as f:
        for name, model, b, rows in cs:
            parts = [name, str(model), str(len(b))] + [float(v).hex() for v in b]
            if rows is not None:
                parts += [str(len(rows))] + [float(v).hex() for v in rows]
            f.write(" ".join(parts) + "\n")


def _doubles(fields):
    v = np.array([float.fromhex(t) for t in fields[1:]], dtype=np.float64)
    assert len(v) == int(fields[0])
    return v


def parse(text):
    """The driver's output as {case name: {field: str | int64 array | float64 array}}; a repeated field (the spliced
    block's msg / ints / vec) gets the suffix 2"""
    res, cur = {}, None
    for line in text.split("\n"):
        if not line:
            continue
        tag, _, rest = line.partition(" ")
        if tag == "case":
            cur = res.setdefault(rest, {})
            continue
        key = tag + "2" if tag in cur else tag
        if tag in ("msg", "splice"):
            cur[key] = rest
        elif tag == "ints":
            cur[key] = np.array([int(t) for t in rest.split()], dtype=np.int64)
        else:
            cur[key] = _doubles(rest.split())
    return res


def run_driver(exe, tmpdir):
    path = os.path.join(tmpdir, "cases.txt")
    cs = cases()
    write_cases(path, cs)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stderr[-4000:]}"
    res = parse(r.stdout)
    assert list(res) == [c[0] for c in cs], "the driver did not print every case once"
    return res


def flatten(res):
    """{"<case>/<field>"}: strings as one joined bytes array, numbers concatenated per dtype with offsets -- a few zip
    members however many cases there are"""
    keys = [f"{c}/{f}" for c in res for f in res[c]]
    vals = [res[c][f] for c in res for f in res[c]]
    out = {"keys": np.array("\n".join(keys).encode()),
           "kind": np.array([0 if isinstance(v, str) else 1 if v.dtype == np.int64 else 2 for v in vals], dtype=np.int8),
           "strs": np.array("\n".join(v for v in vals if isinstance(v, str)).encode())}
    for kind, name, dt in ((1, "ints", np.int64), (2, "dbls", np.float64)):
        arrs = [v for v in vals if not isinstance(v, str) and v.dtype == dt]
        out[name] = np.concatenate(arrs) if arrs else np.zeros(0, dt)
        out[name + "_len"] = np.array([len(a) for a in arrs], dtype=np.int64)
    return out


def unflatten(z):
    keys = z["keys"].item().decode().split("\n")
    strs = iter(z["strs"].item().decode().split("\n"))
    its = {}
    for kind, name in ((1, "ints"), (2, "dbls")):
        its[kind] = iter(np.split(z[name], np.cumsum(z[name + "_len"])[:-1]) if len(z[name + "_len"]) else [])
    res = {}
    for key, kind in zip(keys, z["kind"]):
        c, _, f = key.rpartition("/")
        res.setdefault(c, {})[f] = next(strs) if kind == 0 else next(its[int(kind)])
    return res


def check_messages(res):
    return {f[k] for f in res.values() for k in ("msg", "msg2") if k in f and f[k]}


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/regdata_driver.cpp"
    tmp = str(tmp_path_factory.mktemp("regdata"))
    exe = os.path.join(tmp, "regdata_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "regdata_driver.cpp"), "-o", exe])
    return run_driver(exe, tmp)


def test_cases_cover_every_message_of_the_replaced_checks():
    want = unflatten(np.load(FIXTURE))
    assert [c[0] for c in cases()] == list(want), "the case list no longer matches the recorded fixture"
    assert len(check_messages(want)) == N_CHECK_MESSAGES
    splices = {f["splice"] for f in want.values() if "splice" in f}
    assert len(splices) == 3                            # accepted, header mismatch, shorter than a header
    for m in (GLM, HGLM, CAT, ORD):                     # every model: an accepted image, an accepted spliced image
        assert any("vec" in f and f["ints"][0] == m for f in want.values())
        assert any("vec2" in f and f["ints"][0] == m for f in want.values())


def test_regdata_matches_the_replaced_routines_under_sanitizers(driver_output):
    want = unflatten(np.load(FIXTURE))
    assert list(driver_output) == list(want)
    for name, w in want.items():
        got = driver_output[name]
        assert list(got) == list(w), f"{name}: fields {list(got)} != {list(w)}"
        for field, wv in w.items():
            gv = got[field]
            if isinstance(wv, str):
                assert gv == wv, f"{name}/{field}"
            elif wv.dtype == np.int64:
                assert gv.tolist() == wv.tolist(), f"{name}/{field}"
            else:                                       # bit for bit (NaN payloads and signed zeros included)
                assert gv.shape == wv.shape and (gv.view(np.int64) == wv.view(np.int64)).all(), f"{name}/{field}"


if __name__ == "__main__":                              # record: <driver built against the old routines> <out.npz>
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        rec = run_driver(sys.argv[1], d)
    assert len(check_messages(rec)) == N_CHECK_MESSAGES, sorted(check_messages(rec))
    np.savez_compressed(sys.argv[2], **flatten(rec))
    print(len(rec), "cases ->", sys.argv[2], os.path.getsize(sys.argv[2]), "bytes")
