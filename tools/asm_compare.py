#!/usr/bin/env python3
"""Are two builds' device functions the same code?  tools/asm_compare.py OLD... -- NEW...

Each side is the library's device assembly: one or more .s files, or a directory of them, as `python -m smcnuts_amd.build
--asm DIR` writes them (hipcc -S --cuda-device-only with build.py's flags, one file per unit of build.UNITS).  With two
arguments and no `--` the first is the old side and the second the new one.  A side's functions are the union over its
files, so a build of one unit compares against a build of several, and a kernel that two units instantiate shows up as
a body too many.  A function's body runs from its label to its .Lfunc_end, kernel descriptor included, with
comments dropped and mangled symbols and label numbers replaced by placeholders, so that a renamed template argument or
a shifted function index is no difference.  The multisets of body hashes are compared; nothing but equality is looked at.
Exit status 0 when the function counts agree and no body is on one side only.
"""
import collections, glob, hashlib, os, re, subprocess, sys


def bodies(path):
    text = open(path).read()
    out = []
    for m in re.finditer(r"^(\w+):[^\n]*@\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        lines = (re.sub(r"\s*;.*", "", l).strip() for l in m.group(2).split("\n"))
        body = "\n".join(l for l in lines if l)
        body = re.sub(r"\b_Z\w+", "SYM", body)
        body = re.sub(r"\.(LBB|Ltmp|Lfunc_\w+?)\d+", r".\1N", body)
        out.append((hashlib.sha256(body.encode()).hexdigest(), m.group(1)))
    return out


def read_side(args):
    files = [f for a in args for f in (sorted(glob.glob(os.path.join(a, "*.s"))) if os.path.isdir(a) else [a])]
    return [b for f in files for b in bodies(f)], len(files)


def main(old, new):
    (a, na), (b, nb) = read_side(old), read_side(new)
    ca, cb = collections.Counter(h for h, _ in a), collections.Counter(h for h, _ in b)
    print(f"files: {na} / {nb}; functions: {len(a)} / {len(b)}; distinct bodies: {len(ca)} / {len(cb)}")
    only = [(side, name) for side, fs, rest in (("old", a, ca - cb), ("new", b, cb - ca)) for h, name in fs if h in rest]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in only), capture_output=True, text=True).stdout.split("\n")
    for (side, _), name in zip(only, names):
        print(f"only in {side}: {name}")
    print(f"bodies on one side only: {sum((ca - cb).values())} old, {sum((cb - ca).values())} new")
    return 0 if len(a) == len(b) and not only else 1


if __name__ == "__main__":
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else 1
    sys.exit(main(argv[:cut], [x for x in argv[cut:] if x != "--"]))
