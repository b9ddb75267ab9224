"""In-kernel cycle shares of the NUTS loop (needs a -DSMCN_PROFILE build: SMCN_LIB=...).
    python tools/build_variant.py prof -DSMCN_PROFILE
    SMCN_LIB=smcnuts_amd/variants/libsmcnuts_prof.so python tools/prof_sections.py [steps] [warmup]"""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from smcnuts_amd import ArmaModel, SMCSampler

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
W = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(os.environ.get("PROF_N", "65536"))
smc = SMCSampler(K=W + K, N=N, target=ArmaModel(), step_size=0.01, seed=10, save_history=False)
ctx = smc.samples.ctx
if "PROF_SEGS" in os.environ:      # lane queue: segments per block (0: the launcher's rule)
    ctx.call("smcn_set_lane_segments", int(os.environ["PROF_SEGS"]))
smc.run_fused(upto=W, fuse_max=64)
out = (C.c_uint64 * 16)()
ctx.call("smcn_synchronize")
ctx.call("smcn_debug_profile", out, 1)
ctx.timers(reset=True)
smc.run_fused(upto=W + K, fuse_max=64)
smc.finalise_async()
tm = ctx.timers()
ctx.call("smcn_debug_profile", out, 0)
v = np.array(list(out), dtype=np.float64)
names = ["refill", "leapfrog1", "eval", "leaf tests/first", "park/accept (after 9)", "init block (after 11)", "start-doubling",
         "loop-top", "merge loop", "unwind/top-level", "tree end: take record", "tree end: prefetch + rejoin (after 13)", "tree end: x' stores", "tree end: other stores"]
leaps = smc.leapfrogs[W:].sum()
print(f"nuts launches {int(tm[1])}, {tm[0]:.3f} ms total; leapfrogs {leaps}; {leaps / tm[0] / 1e6:.3f} G leapfrog/s in the kernel")
if os.environ.get("PROF_PHASE"):   # a -DSMCN_PROFILE -DSMCN_PROFILE_PHASE build: the slots are by iteration number mod 4
    book, cnt, inph = v[0:4], v[4:8], v[8:12]
    print(f"wave-iterations: total {v[14]:.0f}, longest wave {v[15]:.0f}; cycles per wave-iteration {(book.sum() + v[12]) / v[14]:.0f}, "
          f"of them draws + leapfrog + evaluation {v[12] / v[14]:.0f}")
    print(f"every live lane's tree began at a multiple of 4: {inph.sum() / cnt.sum() * 100:.2f}% of the wave-iterations")
    print(f"every leaf of the wavefront parks at level 0 (one branch over the rest of the bookkeeping): {v[13] / cnt.sum() * 100:.2f}% "
          f"of the wave-iterations (0 in a build without that path, or with smcn_set_phase_paths(0))")
    out2 = (C.c_uint64 * 16)()
    ctx.call("smcn_debug_profile", out2, 2)      # the second page: slots 16..19, bookkeeping cycles of the in-phase iterations
    bin_ = np.array(list(out2), dtype=np.float64)[0:4]
    for k in range(4):
        print(f"  it mod 4 = {k}: {cnt[k]:12.0f} wave-iterations, in phase {inph[k] / cnt[k] * 100:6.2f}%, "
              f"bookkeeping {book[k] / cnt[k]:7.0f} cycles per wave-iteration: in phase {bin_[k] / max(inph[k], 1):7.0f}, "
              f"not {(book[k] - bin_[k]) / (cnt[k] - inph[k]) if cnt[k] > inph[k] else 0.0:7.0f}")
    # what the launch would cost if every wave-iteration had its residue's in-phase bookkeeping (the evaluation as measured)
    now = (book.sum() + v[12]) / v[14]
    then = (sum(bin_[k] / max(inph[k], 1) * cnt[k] for k in range(4)) + v[12]) / v[14]
    print(f"always in phase: {then:.0f} cycles per wave-iteration against {now:.0f} ({(then / now - 1) * 100:+.2f}%); "
          f"the launch at that rate {tm[0] / max(tm[1], 1) * then / now:.3f} ms against {tm[0] / max(tm[1], 1):.3f}")
    sys.exit(0)
tot = v[:14].sum()
for n, x in zip(names, v[:14]):
    print(f"  {n:18s} {x/tot*100:6.2f}%   {x:.3e}")
if v[14] > 0:
    waves = min(N, 65536) / 64
    print(f"wave-iterations: total {v[14]:.0f}, mean per wave {v[14] / waves:.1f}, longest wave {v[15]:.0f}; "
          f"lane-leapfrogs per wave-iteration {leaps / v[14]:.1f} of 64; cycles per wave-iteration {tot / v[14]:.0f}")
    for n, x in zip(names, v[:14]):
        if x:
            print(f"  {n:28s} {x / v[14]:8.0f} cycles per wave-iteration")
