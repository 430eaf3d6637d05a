#!/usr/bin/env python3
"""Time the soft-input EP E-step (csrc/estep_linear.hip, sbce_estep_prior) and the moments-only
soft-input EP detector call (sbce_detect_linear_prior) with HIP events at estep_ep_bench.py's
shape -- 8x8, P = 65, T_d = 256, 16-QAM, B = 1000 -- beside the prior-free EP arms (sbce_estep,
sbce_detect_linear) on the same buffers in the same process, for every pass count of --passes.
The a-priori L-values are the consistent-Gaussian model at --ia on the true bits.  The arms
alternate call by call, so drift of the machine hits all of them alike; per arm the median, min
and max of --reps calls after --warmup, and per pass count the ratio prior / prior-free of the
medians.  Prints one JSON line.

Usage: python tools/ep_prior_bench.py [--reps 20] [--warmup 3] [--passes 1 5] [--ia 0.5]"""
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
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--ia", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=SHAPE[5])
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    n_tx, n_rx, P, T_d, M, _ = SHAPE
    B = a.batch
    b = with_pilots(pkg, make_batch(pkg, n_tx, n_rx, P, T_d, M, B), n_tx, n_rx, P, 16, M)
    labels = pkg.qam.gray_labeling(M)
    x = np.asarray(b["x_d"] if "x_d" in b else b["x"]).reshape(B, T_d, n_tx)
    idx = np.argmin(np.abs(x[..., None] - np.asarray(b["cons"])), axis=-1)
    bits = pkg.qam.bits_of(labels)[idx]
    la = pkg.qam.prior_llr_gaussian(bits, a.ia, np.random.RandomState(1))
    eng = pkg.EMEngine(b, VARN, mode="ep", prior_llr=la, labels=labels)
    stream = torch.cuda.current_stream().cuda_stream
    mom = eng.mom
    es = float(np.mean(np.abs(b["cons"]) ** 2))

    def dims_ep(p):
        v = {f: getattr(eng.dims, f) for f, _ in L.Dims._fields_}
        v["partition_r"] = p
        return L.Dims(*[v[f] for f, _ in L.Dims._fields_])

    def estep(dims, prior):
        pr = eng.prior.ref() if prior else None
        return lambda: L.check(lib.sbce_estep_prior(dims, eng.ptrs, L.SBCE_ESTEP_EP, pr,
                                                    mom.data_ptr(), stream), "sbce_estep_prior")

    def detect(p, prior):
        d = L.LinearDims(B, n_tx, n_rx, P, T_d, M, L.SBCE_LINEAR_EP, L.linear_ep_passes(p),
                         VARN * VARN, es)
        pt = L.LinearPtrs(y_d=eng.y_d.data_ptr(), psi_d=eng.psi_d.data_ptr(),
                          cons=eng.cons.data_ptr(), theta=eng.theta.data_ptr(),
                          labels=eng.prior.lab.data_ptr(), moments=mom.data_ptr())
        lap = eng.prior.la.data_ptr() if prior else None
        return lambda: L.check(lib.sbce_detect_linear_prior(ctypes.byref(d), ctypes.byref(pt), lap,
                                                            stream), "sbce_detect_linear_prior")

    arms = {}
    for p in a.passes:
        arms[f"estep_ep_p{p}"] = estep(dims_ep(p), False)
        arms[f"estep_ep_prior_p{p}"] = estep(dims_ep(p), True)
        arms[f"detect_ep_p{p}"] = detect(p, False)
        arms[f"detect_ep_prior_p{p}"] = detect(p, True)
    # the prior E-step and the prior detector write the same moments
    p0 = a.passes[-1]
    arms[f"detect_ep_prior_p{p0}"]()
    torch.cuda.synchronize()
    m_d = mom.clone()
    arms[f"estep_ep_prior_p{p0}"]()
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
           "warmup": a.warmup, "ia": a.ia, "moments_max_abs_gap_estep_vs_detect_prior": gap,
           "moments_finite": finite,
           "arms": {k: dict(ms_median=med[k], ms_min=float(np.min(v)), ms_max=float(np.max(v)))
                    for k, v in ms.items()},
           "prior_over_prior_free": {
               **{f"estep_p{p}": med[f"estep_ep_prior_p{p}"] / med[f"estep_ep_p{p}"] for p in a.passes},
               **{f"detect_p{p}": med[f"detect_ep_prior_p{p}"] / med[f"detect_ep_p{p}"]
                  for p in a.passes}}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
