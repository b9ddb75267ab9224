"""smcnuts_amd/build.py: what it compiles, when, and how many at once -- without a compiler.

HIPCC points at a stub this test writes: it appends one JSON line per call (argument vector, start and end stamps) to a
log, writes the `-o` output, and for `-MD` writes the dependency file (`-MF`) listing the unit's source and whatever
`<stub dir>/deps/<unit>` names.  A unit named in `<stub dir>/fail` makes it exit 1 before it writes anything.  build.py
runs on a throw-away copy of the source layout (build.Paths).  Ages are set with os.utime, never waited for: before a
file is touched, everything built so far is moved 10 s into the past.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from smcnuts_amd import build

STUB = r'''#!{python}
import json, os, sys, time
t0 = time.time()
here = os.path.dirname(os.path.abspath(__file__))
a = sys.argv[1:]
src = [x for x in a if x.endswith(".hip")]
unit = os.path.basename(src[0]) if src else ""
time.sleep(float(os.environ.get("STUB_SLEEP", "0")))
fail = os.path.join(here, "fail")
bad = os.path.exists(fail) and unit in open(fail).read().split()
if not bad:
    out = a[a.index("-o") + 1]
    if "-MD" in a:
        extra = os.path.join(here, "deps", unit)
        deps = src + (open(extra).read().split() if os.path.exists(extra) else [])
        open(a[a.index("-MF") + 1], "w").write(out + ": " + " \\\n  ".join(deps) + "\n")
    open(out, "w").write("built from " + " ".join(sorted(os.path.basename(x) for x in a if x.endswith((".hip", ".o")))))
with open(os.path.join(here, "log"), "a") as f:
    f.write(json.dumps({{"argv": a, "unit": unit, "start": t0, "end": time.time()}}) + "\n")
sys.exit(1 if bad else 0)
'''


class Tree:
    def __init__(self, tmp_path, monkeypatch):
        self.stub_dir = tmp_path / "stub"
        (self.stub_dir / "deps").mkdir(parents=True)
        hipcc = self.stub_dir / "hipcc"
        hipcc.write_text(STUB.format(python=sys.executable))
        hipcc.chmod(0o755)
        monkeypatch.setenv("HIPCC", str(hipcc))
        monkeypatch.delenv("MAX_JOBS", raising=False)
        csrc = tmp_path / "pkg" / "csrc"
        csrc.mkdir(parents=True)
        self.common, self.only_predict = csrc / "common.hpp", csrc / "only_predict.hpp"
        self.flags = tmp_path / "pkg" / "build.py"
        for f in [self.common, self.only_predict, self.flags] + [csrc / u for u in build.UNITS]:
            f.write_text("// stand-in\n")
            os.utime(f, (time.time() - 1000, time.time() - 1000))
        for u in build.UNITS:
            listed = [self.common] + ([self.only_predict] if u == "smcn_predict.hip" else [])
            (self.stub_dir / "deps" / u).write_text("\n".join(map(str, listed)))
        self.paths = build.Paths(str(csrc), str(tmp_path / "pkg" / "obj"), str(tmp_path / "pkg" / "libsmcnuts_hip.so"),
                                 str(self.flags))

    def calls(self):
        """(units compiled, links) since the last look; the log is emptied."""
        log = self.stub_dir / "log"
        rows = [json.loads(l) for l in log.read_text().splitlines()] if log.exists() else []
        log.write_text("")
        self.rows = rows
        return sorted(r["unit"] for r in rows if "-c" in r["argv"]), sum("-shared" in r["argv"] for r in rows)

    def touch(self, f):
        """f becomes newer than everything built so far (which moves into the past; its order is kept)."""
        built = [os.path.join(self.paths.objdir, n) for n in os.listdir(self.paths.objdir)] + [self.paths.lib]
        for b in built:
            st = os.stat(b)
            os.utime(b, ns=(st.st_atime_ns, st.st_mtime_ns - 10 * 10**9))
        os.utime(f, (time.time() - 5, time.time() - 5))


@pytest.fixture
def tree(tmp_path, monkeypatch):
    return Tree(tmp_path, monkeypatch)


def test_clean_tree_compiles_every_unit_once_and_links_once(tree):
    assert build.build(paths=tree.paths) == tree.paths.lib
    assert tree.calls() == (sorted(build.UNITS), 1)
    compiles = [r["argv"] for r in tree.rows if "-c" in r["argv"]]
    assert all("--offload-arch=gfx950" in a and "-MD" in a for a in compiles)
    assert open(tree.paths.lib).read() == "built from " + " ".join(sorted(u[:-4] + ".o" for u in build.UNITS))
    # a second call runs nothing
    assert not build.is_stale(tree.paths)
    build.build(paths=tree.paths)
    assert tree.calls() == ([], 0)


def test_a_header_of_one_unit_recompiles_that_unit_alone(tree):
    build.build(paths=tree.paths)
    tree.calls()
    tree.touch(tree.only_predict)
    assert build.stale_units(tree.paths) == ["smcn_predict.hip"]
    build.build(paths=tree.paths)
    assert tree.calls() == (["smcn_predict.hip"], 1)
    build.build(paths=tree.paths)
    assert tree.calls() == ([], 0)
    # a header every unit lists, and the file the flags live in, recompile all of them
    for f in (tree.common, tree.flags):
        tree.touch(f)
        build.build(paths=tree.paths)
        assert tree.calls() == (sorted(build.UNITS), 1)
        build.build(paths=tree.paths)
        assert tree.calls() == ([], 0)


def test_a_missing_dependency_file_or_object_is_stale(tree):
    build.build(paths=tree.paths)
    tree.calls()
    os.remove(os.path.join(tree.paths.objdir, "smcn_loo.o.d"))
    os.remove(os.path.join(tree.paths.objdir, "smcn_summary.o"))
    build.build(paths=tree.paths)
    assert tree.calls() == (["smcn_loo.hip", "smcn_summary.hip"], 1)


def test_a_failed_compile_raises_and_leaves_the_library(tree):
    build.build(paths=tree.paths)
    before = open(tree.paths.lib, "rb").read()
    mtime = os.stat(tree.paths.lib).st_mtime_ns
    tree.calls()
    (tree.stub_dir / "fail").write_text("smcn_predict.hip")
    tree.touch(tree.flags)
    mtime -= 10 * 10**9
    with pytest.raises(subprocess.CalledProcessError):
        build.build(paths=tree.paths)
    units, links = tree.calls()
    assert "smcn_predict.hip" in units and links == 0
    assert open(tree.paths.lib, "rb").read() == before and os.stat(tree.paths.lib).st_mtime_ns == mtime
    assert build.is_stale(tree.paths)
    # ... and the next build, with the compiler mended, redoes at least the failed unit and links
    (tree.stub_dir / "fail").unlink()
    build.build(paths=tree.paths)
    units, links = tree.calls()
    assert "smcn_predict.hip" in units and links == 1 and not build.is_stale(tree.paths)


def test_max_jobs_bounds_the_compiles_in_flight(tree, monkeypatch):
    monkeypatch.setenv("MAX_JOBS", "2")
    monkeypatch.setenv("STUB_SLEEP", "0.1")
    build.build(paths=tree.paths)
    assert tree.calls() == (sorted(build.UNITS), 1)
    spans = [(r["start"], r["end"]) for r in tree.rows if "-c" in r["argv"]]
    in_flight = max(sum(s <= t < e for s, e in spans) for t, _ in spans)
    assert in_flight <= 2
    link = next(r for r in tree.rows if "-shared" in r["argv"])
    assert link["start"] >= max(e for _, e in spans)          # one link, behind the last compile
