#!/usr/bin/env python3
"""Time the expectation-propagation E-step (csrc/estep_linear.hip) and the moments-only EP detector
call with HIP events at 8x8, P = 65, T_d = 256, 16-QAM, B = 1000, beside the soft MMSE E-step and
the moments-only MMSE detector call on the same buffers in the same process.  One arm per pass
count of --passes for the E-step, the default pass count for the detector.  The arms alternate
call by call, so drift of the machine hits all of them alike; per arm the median, min and max of
--reps calls after --warmup, and for every EP arm its ratio to p x the soft MMSE E-step's median of
the same run (staging is done once and a pass is at most one MMSE solve plus demap, so the ratio
should not exceed 1).  Prints one JSON line.

Usage: python tools/estep_ep_bench.py [--reps 20] [--warmup 3] [--passes 1 2 5 16]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
from detect_bench import make_batch, VARN  # noqa: E402
from estep_linear_bench import SHAPE, with_pilots  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 2, 5, 16])
    ap.add_argument("--batch", type=int, default=SHAPE[5])
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    n_tx, n_rx, P, T_d, M, _ = SHAPE
    B = a.batch
    b = with_pilots(pkg, make_batch(pkg, n_tx, n_rx, P, T_d, M, B), n_tx, n_rx, P, 16, M)
    eng = pkg.EMEngine(b, VARN, mode="mmse_soft")
    stream = torch.cuda.current_stream().cuda_stream
    mom = eng.mom
    es = float(np.mean(np.abs(b["cons"]) ** 2))

    def dims_ep(p):
        v = {f: getattr(eng.dims, f) for f, _ in L.Dims._fields_}
        v["partition_r"] = p
        return L.Dims(*[v[f] for f, _ in L.Dims._fields_])

    def estep(dims, mode):
        return lambda: L.check(lib.sbce_estep(dims, eng.ptrs, mode, mom.data_ptr(), stream),
                               "sbce_estep")

    def detect(kind, flags):
        d = L.LinearDims(B, n_tx, n_rx, P, T_d, M, kind, flags, VARN * VARN, es)
        p = L.LinearPtrs(y_d=eng.y_d.data_ptr(), psi_d=eng.psi_d.data_ptr(),
                         cons=eng.cons.data_ptr(), theta=eng.theta.data_ptr(),
                         moments=mom.data_ptr())
        return lambda: L.check(lib.sbce_detect_linear(ctypes.byref(d), ctypes.byref(p), stream),
                               "sbce_detect_linear")

    arms = {"estep_mmse_soft": estep(eng.dims, L.SBCE_ESTEP_MMSE_SOFT)}
    for p in a.passes:
        arms[f"estep_ep_p{p}"] = estep(dims_ep(p), L.SBCE_ESTEP_EP)
    arms["detect_linear_moments_mmse"] = detect(L.SBCE_LINEAR_MMSE, 0)
    arms["detect_linear_moments_ep_p5"] = detect(L.SBCE_LINEAR_EP, 0)
    # the E-step and the detector write the same EP moments (es = 10 on the host and the device)
    arms["detect_linear_moments_ep_p5"]()
    torch.cuda.synchronize()
    m_d = mom.clone()
    estep(dims_ep(0), L.SBCE_ESTEP_EP)()
    torch.cuda.synchronize()
    gap = float((mom - m_d).abs().max().item())
    finite = bool(torch.isfinite(mom.abs()).all().item())
    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"shape": dict(n_tx=n_tx, n_rx=n_rx, P=P, T_d=T_d, M=M, batch=B), "reps": a.reps,
           "warmup": a.warmup, "moments_max_abs_gap_estep_vs_detect_ep": gap,
           "moments_finite": finite,
           "arms": {k: dict(ms_median=med[k], ms_min=float(np.min(v)), ms_max=float(np.max(v)))
                    for k, v in ms.items()},
           "ep_over_p_times_mmse_soft": {str(p): med[f"estep_ep_p{p}"] / (p * med["estep_mmse_soft"])
                                         for p in a.passes}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
