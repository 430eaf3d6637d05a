"""Diagnostic: tile groups of the V16 sweep per listed symbol on one cfg1 sub-batch (334 trials):
groups that reach the FP32 screen (sbce_debug_estep_groups) and FP64 groups (FP64 MFMAs / 8), at
theta_0 (the iteration-0 E-step) and after a 20-iteration EM, under alternating settings, with
the E-step's time by HIP events (median of REPS), e.g.
  python tools/estep_groups.py SBCE_ESTEP_TRI=0 SBCE_ESTEP_TRI=1 SBCE_ESTEP_TRI=2
  python tools/estep_groups.py SBCE_ESTEP_ORDER=1 SBCE_ESTEP_ORDER=0        (best-first / natural order)
  python tools/estep_groups.py SBCE_ESTEP_TWOPASS=1 SBCE_ESTEP_TWOPASS=0    (two-pass / one-pass sweep)
"second pass" is the tile groups the two-pass sweep's second pass recomputed (sbce_debug_estep_pass2).
One K=V per arm; a second switch of a combined arm is set in the environment of the run."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

pkg = ge.package()
pkg._lib.use_ab()       # the A/B build: SBCE_* switches, counters
B = int(os.environ.get("TRIALS", "334"))
reps = int(os.environ.get("REPS", "5"))
varn = float(pkg.signal_model.snr_to_varn(float(os.environ.get("SNR", "20"))))
batch = pkg.signal_model.synthetic_batch(B, 4, 4, 64, 16, 256, 16, varn, seed=0)
eng = pkg.EMEngine(batch, varn)
lib = pkg._lib.load()
nsym = B * 256


def measure(arm):
    k, v = arm.split("=", 1)
    os.environ[k] = v
    os.environ["SBCE_ESTEP_COUNT"] = "1"
    pkg._lib.reload_debug_env()
    grp, mf = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    sph = (ctypes.c_ulonglong * 3)()
    have_groups = hasattr(lib, "sbce_debug_estep_groups")     # absent before the per-group bounds
    if have_groups:
        lib.sbce_debug_estep_groups(None, 1)
    have_pass2 = hasattr(lib, "sbce_debug_estep_pass2")       # absent before the two-pass sweep
    p2 = ctypes.c_ulonglong(0)
    if have_pass2:
        lib.sbce_debug_estep_pass2(None, 1)
    lib.sbce_debug_estep_mfma(None, 1)
    lib.sbce_debug_estep_sphere(None, 1)
    lib.sbce_debug_estep_pair(None, 1)
    npair = ctypes.c_ulonglong(0)
    eng.estep()
    torch.cuda.synchronize()
    if have_groups:
        lib.sbce_debug_estep_groups(ctypes.byref(grp), 0)
    lib.sbce_debug_estep_mfma(ctypes.byref(mf), 0)
    if have_pass2:
        lib.sbce_debug_estep_pass2(ctypes.byref(p2), 0)
    lib.sbce_debug_estep_sphere(sph, 0)
    lib.sbce_debug_estep_pair(ctypes.byref(npair), 0)
    del os.environ["SBCE_ESTEP_COUNT"]
    pkg._lib.reload_debug_env()
    ms = []
    for _ in range(reps):        # timed without the counters' atomics
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.estep()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del os.environ[k]
    pkg._lib.reload_debug_env()
    swept = int(sph[1]) - npair.value if os.environ.get("SBCE_ESTEP_SPHERE") != "0" else nsym
    return swept, grp.value, mf.value // 8, p2.value, float(np.median(ms))


for label, its in (("theta_0", 0), ("after 20 EM its", 20)):
    if its:
        eng.run(its)
        torch.cuda.synchronize()
    for arm in sys.argv[1:] or ["SBCE_ESTEP_TRI=1"]:
        swept, grp, g64, g2, ms = measure(arm)
        n = max(swept, 1)
        print(f"{label:16s} {arm:18s} listed {swept:6d} of {nsym}  to screen {grp / n:6.2f}  "
              f"FP64 groups {g64 / n:6.2f}  second pass {g2 / n:5.2f} per listed symbol   "
              f"E-step {ms:7.3f} ms", flush=True)
