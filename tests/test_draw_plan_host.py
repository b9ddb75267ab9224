"""What smcn_predict_draws and smcn_forecast_draws share on the host (smcnuts_amd/csrc/smcn_draw_plan.hpp) under the
address and undefined-behaviour sanitizers.

tests/draw_plan_driver.cpp (a stand-alone program that includes only the header) is compiled with
`g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run once.  It exits non-zero unless, for every M in
{1, 15, 16, 17, 1023, 1024, 1025, 2049} and n in {1, 16, 17}, the work area's offsets equal the formulas the two entry
points spelled out before they shared the plan (restated there as literal arithmetic), no two regions overlap and
nt = ceil(M / 1024); each refusal is produced by its smallest triggering input with its exact text, for "draws" and for
"paths", and several faults at once report the first in the entry points' order; and the NaN count is right on an array
with NaNs first, last and nowhere.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_plan_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/draw_plan_driver.cpp"
    exe = str(tmp_path / "draw_plan_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "draw_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.strip() == "draw plan ok"
