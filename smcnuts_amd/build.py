"""Build libsmcnuts_hip.so (hipcc, gfx950) in-tree: one object per unit, compiled side by side, one link."""
import collections
import concurrent.futures
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# The library's translation units (csrc/smcn_ctx.hpp: who owns which kernels).  The core is the longest compile.
UNITS = ["smcn_api.hip", "smcn_loo.hip", "smcn_predict.hip", "smcn_summary.hip", "smcn_forecast.hip"]
LIB = os.path.join(HERE, "libsmcnuts_hip.so")

# Where a build reads and writes.  `flags_file` is this file: the compiler flags live here, so it dates every object.
Paths = collections.namedtuple("Paths", "csrc objdir lib flags_file")
DEFAULT = Paths(os.path.join(HERE, "csrc"), os.path.join(HERE, "obj"), LIB, os.path.abspath(__file__))


def hipcc_cmd(src, out, defines=(), asm_only=False, verbose=False):
    """The compile line of one unit: an object with its dependency file beside it (<out minus .tmp>.d), or, asm_only, the
    unit's device assembly.  The flags are spelled here and nowhere else."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -amdgpu-atomic-optimizer-strategy=None: the work-queue atomics of the NUTS kernel are issued
    # per particle group and consumed one tree later; the wave-aggregating optimizer would wait for
    # the result at once (readfirstlane), exposing the atomic's round trip on every claim.
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", *defines]
    if verbose:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    if asm_only:
        return cmd + ["-S", "--cuda-device-only", "-o", out, src]
    return cmd + ["-fPIC", "-c", "-MD", "-MF", _stem(out) + ".d", "-o", out, src]


def link_cmd(objs, out):
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-shared", "-fPIC", "-o", out, *objs, "-ldl"]


def _stem(obj):
    return obj[:-len(".tmp")] if obj.endswith(".tmp") else obj


def _obj(paths, unit):
    return os.path.join(paths.objdir, os.path.splitext(unit)[0] + ".o")


def _dep_files(dfile):
    """The prerequisites a compiler-written dependency file lists (make syntax: `target: a b \\`)."""
    text = open(dfile).read().replace("\\\n", " ")
    return text.split(":", 1)[1].split() if ":" in text else []


def object_is_stale(paths, unit):
    """Missing, without its dependency file, or older than anything that file lists or than the flags."""
    obj = _obj(paths, unit)
    if not os.path.exists(obj) or not os.path.exists(obj + ".d"):
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in _dep_files(obj + ".d") + [paths.flags_file])


def stale_units(paths=DEFAULT):
    return [u for u in UNITS if object_is_stale(paths, u)]


def is_stale(paths=DEFAULT):
    if not os.path.exists(paths.lib) or stale_units(paths):
        return True
    t = os.path.getmtime(paths.lib)
    return any(os.path.getmtime(_obj(paths, u)) > t for u in UNITS)


def build(force=False, verbose=False, paths=DEFAULT, defines=()):
    """hipcc --offload-arch=gfx950 -> smcnuts_amd/libsmcnuts_hip.so (cross-compiles without a GPU)."""
    if not force and not is_stale(paths):
        return paths.lib
    import fcntl
    with open(paths.lib + ".lock", "w") as lock:     # several ranks may get here at once: one builds, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not is_stale(paths):
            return paths.lib
        return _compile(paths, UNITS if force else stale_units(paths), verbose, defines)


def _compile_unit(paths, unit, verbose, defines):
    obj = _obj(paths, unit)
    subprocess.check_call(hipcc_cmd(os.path.join(paths.csrc, unit), obj + ".tmp", defines, verbose=verbose))
    os.replace(obj + ".tmp", obj)                    # (an interrupted compile leaves no object that looks fresh)


def _compile(paths, units, verbose, defines):
    os.makedirs(paths.objdir, exist_ok=True)
    jobs = max(1, min(len(UNITS), int(os.environ.get("MAX_JOBS", "16"))))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for done in [pool.submit(_compile_unit, paths, u, verbose, defines) for u in units]:
            done.result()                            # a failed compile raises here, before anything touches the library
    tmp = paths.lib + ".tmp"
    subprocess.check_call(link_cmd([_obj(paths, u) for u in UNITS], tmp))
    os.replace(tmp, paths.lib)                       # atomic: a reader never sees a half-written library
    return paths.lib


def device_asm(outdir, defines=()):
    """The device assembly of every unit, <outdir>/<unit>.s (tools/dis_kernel.sh, tools/asm_compare.py)."""
    os.makedirs(outdir, exist_ok=True)
    outs = [os.path.join(outdir, os.path.splitext(u)[0] + ".s") for u in UNITS]
    jobs = max(1, min(len(UNITS), int(os.environ.get("MAX_JOBS", "16"))))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        list(pool.map(lambda uo: subprocess.check_call(hipcc_cmd(os.path.join(DEFAULT.csrc, uo[0]), uo[1], defines, asm_only=True)),
                      zip(UNITS, outs)))
    return outs


if __name__ == "__main__":
    if sys.argv[1:2] == ["--asm"]:                   # python -m smcnuts_amd.build --asm DIR [-DNAME ...]
        print("\n".join(device_asm(sys.argv[2], sys.argv[3:])))
    else:
        print(build(force=True))
