#!/usr/bin/env python3
"""Time the Cramer-Rao bound call (csrc/crb.hip) with HIP events at the cfg1 shape (4x4, P = 65,
T_p = 16, T_d = 256, 16-QAM, B = 1000, the bench's data at 20 dB), beside the M-step for scale:
  * one sbce_crb call (the M-step's build launches, then the factor / inverse / norms kernel) on
    the moments of one SOFT E-step at theta_0, and on the genie moments x x^H;
  * the build launches alone (sbce_debug_mstep_phase 2: R and B^H), so that the difference is the
    new kernel's share;
  * one sbce_mstep call (build + Cholesky solve) on the same moments, in the same process.
Warm-up calls first, then --reps timed calls each; prints one JSON line with median, min and max.

Usage: python tools/crb_bench.py [--reps 10] [--warmup 2] [--batch 1000]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

N_TX, N_RX, N_RIS, T_P, T_D, M = 4, 4, 64, 16, 256, 16


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.asarray(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1000)
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    B = a.batch
    varn = float(pkg.signal_model.snr_to_varn(20.0))
    batch = pkg.signal_model.synthetic_batch(B, N_TX, N_RX, N_RIS, T_P, T_D, M, varn, seed=0)
    eng = pkg.EMEngine(batch, varn, mode="soft", x_d_true=batch["x_d"])
    del batch
    stream = torch.cuda.current_stream().cuda_stream
    nb = ctypes.c_size_t(0)
    L.check(lib.sbce_crb_workspace_bytes(ctypes.byref(eng.dims), ctypes.byref(nb)), "bytes")
    scratch = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    n_l = eng.P * eng.n_tx
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    tr, diag, mse, bound = f64(B), f64(B, n_l), f64(B), f64(B)
    ptrs = L.Ptrs.from_buffer_copy(eng.ptrs)
    ptrs.h_true = eng.h.data_ptr()
    opts = L.CrbOpts(varn, None, tr.data_ptr(), diag.data_ptr(), mse.data_ptr(), bound.data_ptr(),
                     scratch.data_ptr(), scratch.numel(), 0)
    eng.estep()                                        # moments of theta_0
    x = eng.x_d
    genie = torch.cat([x, (x[..., :, None] * x[..., None, :].conj()).reshape(B, T_D, -1)],
                      dim=2).contiguous()

    def crb(mom):
        L.check(lib.sbce_crb(eng.dims, ptrs, mom.data_ptr(), opts, stream), "sbce_crb")

    t_em = timed(torch, lambda: crb(eng.mom), a.warmup, a.reps)
    em = dict(bound_mean=float(bound.mean().item()), flagged=int((eng.status != 0).sum().item()))
    t_ge = timed(torch, lambda: crb(genie), a.warmup, a.reps)
    ge = dict(bound_mean=float(bound.mean().item()), bound_max=float(bound.max().item()),
              flagged=int((eng.status != 0).sum().item()))
    t_build = timed(torch, lambda: eng.mstep_phase(2), a.warmup, a.reps)
    t_mstep = timed(torch, eng.mstep, a.warmup, a.reps)
    flops = 4.0 * 2.0 * n_l ** 3 / 3.0 * B             # factor + triangular inverse, complex MACs as 8 flops
    print(json.dumps({
        "shape": "cfg1", "n_tx": N_TX, "n_rx": N_RX, "P": N_RIS + 1, "L": n_l, "T_p": T_P, "T_d": T_D,
        "M": M, "batch": B, "reps": a.reps, "warmup": a.warmup, "varn": varn,
        "crb_em_moments": t_em, "crb_genie_moments": t_ge, "build_only": t_build, "mstep": t_mstep,
        "crb_kernel_ms_by_difference": t_em["ms_median"] - t_build["ms_median"],
        "crb_kernel_nominal_GFLOPs": flops / max(t_em["ms_median"] - t_build["ms_median"], 1e-9) / 1e6,
        "em": em, "genie": ge,
    }), flush=True)


if __name__ == "__main__":
    main()
