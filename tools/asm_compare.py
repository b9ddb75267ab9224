#!/usr/bin/env python3
"""Are two builds' device functions the same code?  tools/asm_compare.py old.s new.s

Each input is the library's device assembly: tools/dis_kernel.sh's hipcc line (-S --cuda-device-only with build.py's
flags) on csrc/smcn_api.hip.  A function's body runs from its label to its .Lfunc_end, kernel descriptor included, with
comments dropped and mangled symbols and label numbers replaced by placeholders, so that a renamed template argument or
a shifted function index is no difference.  The multisets of body hashes are compared; nothing but equality is looked at.
Exit status 0 when the function counts agree and no body is on one side only.
"""
import collections, hashlib, re, subprocess, sys


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


def main(old, new):
    a, b = bodies(old), bodies(new)
    ca, cb = collections.Counter(h for h, _ in a), collections.Counter(h for h, _ in b)
    print(f"functions: {len(a)} / {len(b)}; distinct bodies: {len(ca)} / {len(cb)}")
    only = [(side, name) for side, fs, rest in (("old", a, ca - cb), ("new", b, cb - ca)) for h, name in fs if h in rest]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in only), capture_output=True, text=True).stdout.split("\n")
    for (side, _), name in zip(only, names):
        print(f"only in {side}: {name}")
    print(f"bodies on one side only: {sum((ca - cb).values())} old, {sum((cb - ca).values())} new")
    return 0 if len(a) == len(b) and not only else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
