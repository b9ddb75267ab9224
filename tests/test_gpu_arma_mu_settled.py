"""smcn_selftest_recur: the arma recurrence the kernels run (mu-sensitivity no longer updated once it repeats with period
<= 2 on every executing lane of a wavefront; smcn_nuts3.hpp) against the full recurrence in the same
binary, bit for bit, on wavefronts composed row by row; the switch step of every wavefront against the exact emulation of
tests/_arma_recur.py."""
import json
import os

import numpy as np
import pytest

from _arma_recur import expected_switch, recur_float, settle_step, two_cycle_thetas

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "smcnuts_amd", "model", "data")
BETA = 0.957
NAN_ROW, BIG_ROW, MID_ROW, CYC_ROW = 4 * 64 + 11, 3 * 64 + 40, 64 + 5, 2 * 64 + 63
N_ROWS = 5 * 64 + 37


@pytest.fixture(scope="module")
def rows():
    """Six wavefronts, 64 rows each in row order (the last one ragged), and the exact settle step of every row."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(N_ROWS, 4)) * np.array([0.05, 0.05, 0.0, 0.1]) + np.array([0, 0.9, 0, -1.8])
    x[:, 2] = rng.uniform(-0.1, 0.1, size=N_ROWS)              # block 0 (and everything not set below): |theta| <= 0.1
    x[MID_ROW, 2] = -0.45                                      # block 1: one slow lane among fast ones
    cyc = two_cycle_thetas(BETA, 1, hi=0.2)[0]                 # block 2: a theta > 0 lane that ends in a genuine 2-cycle
    x[CYC_ROW, 1:3] = BETA, cyc
    x[BIG_ROW, 2] = 1.05                                       # block 3: one lane beyond the unit circle
    x[NAN_ROW, 2] = np.nan                                     # block 4: one NaN lane
    settle = [settle_step(float(r[2]), float(r[1]), 400) for r in x]
    assert settle[CYC_ROW][1] == 2 and settle[CYC_ROW][0] <= 32
    assert 32 < settle[MID_ROW][0] <= 64
    assert settle[BIG_ROW][0] is None and settle[NAN_ROW][0] is None
    return x, [s[0] for s in settle]


@pytest.mark.parametrize("T", [1, 2, 17, 32, 33, 34, 49, 64, 65, 97, 137, 200, 383])
def test_shipped_recurrence_is_the_full_one_bit_for_bit(tmp_path, rows, T):
    from smcnuts_amd import ArmaModel, _capi
    x, settle = rows
    src = json.load(open(os.path.join(DATA, "arma.json")))
    y = (src["y"] * 2)[:T]
    path = str(tmp_path / "arma_T.json")
    json.dump({"T": T, "y": y}, open(path, "w"))
    t = ArmaModel(path)
    ctx = _capi.Context(64, t.model_id, t.model_data)
    out = np.full((N_ROWS, 9), -7.0)
    ctx.call("smcn_selftest_recur", _capi.dptr(np.ascontiguousarray(x)), N_ROWS, _capi.dptr(out))
    full, shipped, sw = out[:, :4], out[:, 4:8], out[:, 8]
    print(f"T={T} switch steps per wavefront: {sw[::64].tolist()}")
    # the shipped form gives the full form's bits, the NaN lane's NaNs included
    np.testing.assert_array_equal(np.ascontiguousarray(shipped).view(np.uint64), np.ascontiguousarray(full).view(np.uint64))
    assert np.all(np.isfinite(np.delete(full, NAN_ROW, axis=0)))
    assert np.all(np.isnan(full[NAN_ROW])) or T == 1               # (one observation: no step, theta is not read)
    # the switch step is wave-uniform and the one the exact emulation of the mu-sensitivity gives
    want = [expected_switch(settle[b:b + 64], T) for b in range(0, N_ROWS, 64)]
    for b, w in enumerate(want):
        np.testing.assert_array_equal(sw[64 * b:64 * b + 64], w, err_msg=f"wavefront {b}")
    if T >= 33:
        assert want[0] == 32 and want[2] == 32 and want[5] == 32     # fast lanes, a 2-cycle lane among them, the ragged block
        assert want[1] == (64 if T >= 65 else 0)                     # the slow lane holds its wavefront back one more trip
    else:
        assert want[:3] == [0, 0, 0] and want[5] == 0                # too short to reach a test
    assert want[3] == 0 and want[4] == 0                             # |theta| >= 1, NaN: never
    # both forms against the host recurrence in extended precision
    ok = np.arange(N_ROWS) != NAN_ROW
    ref = recur_float(y, x[ok])
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1.0            # the sensitivity sums cancel against each other
    for got in (full[ok], shipped[ok]):
        assert np.max(np.abs(got - ref) / scale) < 1e-12, np.max(np.abs(got - ref) / scale)
