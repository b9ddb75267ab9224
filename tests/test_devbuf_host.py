"""The owner types of a context's device buffers and timing events (smcnuts_amd/csrc/smcn_devbuf.hpp) under the address
and undefined-behaviour sanitizers.

tests/devbuf_driver.cpp (a stand-alone program that includes only the header, with an allocator that counts and can
fail the k-th request) is compiled with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run once.  It
exits non-zero unless, at 0, 1, 2 and 3 elements: growing within the length calls nothing and keeps the pointer; growing
beyond it frees the old block once, before the new request; a failed request leaves (null, 0) and the next, smaller one
allocates again; a reset at the same size frees and allocates; moves leave the source empty; everything is freed exactly
once; an event is created at its first use and destroyed once.  That a buffer cannot be copied is a static_assert.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_rules_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/devbuf_driver.cpp"
    exe = str(tmp_path / "devbuf_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "devbuf_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.strip() == "devbuf ok"
