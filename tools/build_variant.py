"""Diagnostic builds of the library (same ABI), kept out of the product .so:
    python tools/build_variant.py <tag> [-DNAME ...]   ->  smcnuts_amd/variants/libsmcnuts_<tag>.so
The defines are the diagnostic switches of the sources: -DSMCN_PROFILE (and -DSMCN_PROFILE_TAIL=n), the in-kernel
section profile tools/prof_sections*.py read; -DSMCN_TRACE_SETUP, where a context's set-up time goes.
Load one with SMCN_LIB=<path>.  Units, flags and staleness are smcnuts_amd/build.py's; a variant has its own objects."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smcnuts_amd import build
tag, defs = sys.argv[1], sys.argv[2:]
out = os.path.join(ROOT, "smcnuts_amd", "variants", f"libsmcnuts_{tag}.so")
os.makedirs(os.path.dirname(out), exist_ok=True)
paths = build.DEFAULT._replace(objdir=os.path.join(build.DEFAULT.objdir, f"variant_{tag}"), lib=out)
print(build.build(force=True, paths=paths, defines=defs))
