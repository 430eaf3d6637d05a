#!/usr/bin/env python3
"""Time the soft MMSE E-step (csrc/estep_linear.hip) with HIP events at 8x8, P = 65, T_d = 256,
16-QAM, B = 1000, beside the two calls it is to be compared with on the same buffers:
sbce_detect_linear asked for the moments only (the same arithmetic plus its zeroing launch and
label work) and the hard SBCE_ESTEP_MMSE E-step.  --other-lib PATH adds the same two calls from
another build of libsbce.so (the parent commit's) as arms of their own.  The arms alternate call by
call inside one process, so drift of the machine hits all of them alike; per arm the median, min
and max of --reps calls after --warmup.  Then one EM run (EMEngine, mode mmse_soft, --itera
iterations, T_p = --t-p Kronecker pilots) gives the end-to-end time per iteration.
Prints one JSON line.

Usage: python tools/estep_linear_bench.py [--reps 20] [--warmup 3] [--other-lib PATH]"""
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

SHAPE = (8, 8, 65, 256, 16, 1000)        # n_tx, n_rx, P, T_d, M, B


def with_pilots(pkg, b, n_tx, n_rx, P, T_p, M, seed=1):
    """make_batch's trials with T_p Kronecker pilots u_p = psi_p (x) x_p observed through theta0's
    channel (the E-step timings do not read them; the EM run's M-step does)."""
    r = np.random.RandomState(seed)
    B = b["y_d"].shape[0]
    cons = b["cons"]
    psi_p = np.exp(2j * np.pi * r.uniform(size=(B, T_p, P)))
    x_p = cons[r.randint(0, M, size=(B, T_p, n_tx))]
    u_p = (psi_p[:, :, :, None] * x_p[:, :, None, :]).reshape(B, T_p, P * n_tx)
    y_p = np.einsum("btl,blr->btr", u_p, b["theta0"].reshape(B, P * n_tx, n_rx))
    y_p = y_p + np.sqrt(VARN / 2) * (r.randn(*y_p.shape) + 1j * r.randn(*y_p.shape))
    return dict(b, u_p=u_p, y_p=y_p)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--itera", type=int, default=20)
    ap.add_argument("--t-p", type=int, default=16)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--batch", type=int, default=SHAPE[5])
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    n_tx, n_rx, P, T_d, M, _ = SHAPE
    B = a.batch
    b = with_pilots(pkg, make_batch(pkg, n_tx, n_rx, P, T_d, M, B), n_tx, n_rx, P, a.t_p, M)
    eng = pkg.EMEngine(b, VARN, mode="mmse_soft")
    stream = torch.cuda.current_stream().cuda_stream
    mom = eng.mom
    es = float(np.mean(np.abs(b["cons"]) ** 2))
    ldims = L.LinearDims(B, n_tx, n_rx, P, T_d, M, L.SBCE_LINEAR_MMSE, 0, VARN * VARN, es)
    lptrs = L.LinearPtrs(y_d=eng.y_d.data_ptr(), psi_d=eng.psi_d.data_ptr(),
                         cons=eng.cons.data_ptr(), theta=eng.theta.data_ptr(),
                         moments=mom.data_ptr())

    def estep(lib, mode):
        return lambda: L.check(lib.sbce_estep(eng.dims, eng.ptrs, mode, mom.data_ptr(), stream),
                               "sbce_estep")

    def detect(lib):
        return lambda: L.check(lib.sbce_detect_linear(ctypes.byref(ldims), ctypes.byref(lptrs),
                                                      stream), "sbce_detect_linear")

    here = L.load()
    arms = {"estep_mmse_soft": estep(here, L.SBCE_ESTEP_MMSE_SOFT),
            "detect_linear_moments": detect(here),
            "estep_mmse_hard": estep(here, L.SBCE_ESTEP_MMSE)}
    if a.other_lib:
        other = L.load(os.path.abspath(a.other_lib))
        arms["other_detect_linear_moments"] = detect(other)
        arms["other_estep_mmse_hard"] = estep(other, L.SBCE_ESTEP_MMSE)
    # the two soft arms write the same moments, up to es formed on the host / on the device
    arms["estep_mmse_soft"]()
    torch.cuda.synchronize()
    m_e = mom.clone()
    arms["detect_linear_moments"]()
    torch.cuda.synchronize()
    gap = float((mom - m_e).abs().max().item())
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
    out = {"shape": dict(n_tx=n_tx, n_rx=n_rx, P=P, T_d=T_d, M=M, batch=B), "reps": a.reps,
           "warmup": a.warmup, "moments_max_abs_gap_estep_vs_detect": gap,
           "arms": {k: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)),
                            ms_max=float(np.max(v))) for k, v in ms.items()}}
    # end to end: one whole EM, host clock around work that ends in a synchronise
    import time
    eng.run(2)
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.run(a.itera)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    out["em_mmse_soft"] = dict(itera=a.itera, t_p=a.t_p, ms_per_run=runs,
                               ms_per_iteration_median=float(np.median(runs)) / a.itera,
                               finite=bool(torch.isfinite(eng.theta.abs()).all().item()),
                               status_or=int(np.bitwise_or.reduce(eng.status.cpu().numpy())))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
