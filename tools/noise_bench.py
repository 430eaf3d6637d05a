#!/usr/bin/env python3
"""Time the noise-variance update (csrc/noise.hip) with HIP events at the cfg1 shape (4x4, P = 65,
T_p = 16, T_d = 256, 16-QAM, B = 1000, the bench's data at 20 dB):
  * one sbce_noise_var call (both launches) from theta_0 and the moments of one SOFT E-step;
  * a device-to-device copy of the byte count the update reads once (psi_d, moments, y_d, y_p, u_p,
    theta), timed in the same process: the bandwidth yardstick (a copy also WRITES that many bytes);
  * sbce_em_noise against sbce_em on the same inputs, per iteration (--iters iterations per call),
    with the mean NMSE each leaves.
Warm-up calls first, then --reps timed calls each; prints one JSON line with median, min and max.

Usage: python tools/noise_bench.py [--reps 10] [--warmup 2] [--iters 5] [--batch 1000]"""
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1000)
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    B = a.batch
    varn = float(pkg.signal_model.snr_to_varn(20.0))
    batch = pkg.signal_model.synthetic_batch(B, N_TX, N_RX, N_RIS, T_P, T_D, M, varn, seed=0)
    eng = pkg.EMEngine(batch, varn, mode="soft")
    del batch
    stream = torch.cuda.current_stream().cuda_stream
    nb = ctypes.c_size_t(0)
    L.check(lib.sbce_noise_workspace_bytes(ctypes.byref(eng.dims), ctypes.byref(nb)), "bytes")
    scratch = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    est = torch.zeros(B, dtype=torch.float64, device="cuda")
    hist = torch.zeros((B, a.iters), dtype=torch.float64, device="cuda")
    opts = L.NoiseOpts(est.data_ptr(), hist.data_ptr(), scratch.data_ptr(), scratch.numel(), 1e-6, 0)
    eng.estep()                                        # moments of theta_0

    def noise_var():
        L.check(lib.sbce_noise_var(eng.dims, eng.ptrs, eng.mom.data_ptr(), opts, stream),
                "sbce_noise_var")

    read = sum(t.numel() * t.element_size()
               for t in (eng.psi_d, eng.mom, eng.y_d, eng.y_p, eng.u_p, eng.theta))
    src = torch.empty(read, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def em():
        eng.theta.copy_(eng.theta0)
        L.check(lib.sbce_em(eng.dims, eng.ptrs, a.iters, eng.mode, eng.solve, stream), "sbce_em")

    def em_noise():
        eng.theta.copy_(eng.theta0)
        L.check(lib.sbce_em_noise(eng.dims, eng.ptrs, a.iters, eng.mode, eng.solve, opts, stream),
                "sbce_em_noise")

    t_nv = timed(torch, noise_var, a.warmup, a.reps)
    s2 = (est * est).cpu().numpy()
    t_cp = timed(torch, lambda: dst.copy_(src), a.warmup, a.reps)
    t_em = timed(torch, em, a.warmup, a.reps)
    nmse_em = float(eng.nmse().mean().item())
    t_en = timed(torch, em_noise, a.warmup, a.reps)
    nmse_en = float(eng.nmse().mean().item())
    s2_em = (est * est).cpu().numpy()
    print(json.dumps({
        "shape": "cfg1", "n_tx": N_TX, "n_rx": N_RX, "P": N_RIS + 1, "T_p": T_P, "T_d": T_D, "M": M,
        "batch": B, "reps": a.reps, "warmup": a.warmup, "iters": a.iters, "varn_true": varn,
        "noise_var": t_nv, "bytes_read": read, "d2d_copy_same_bytes": t_cp,
        "noise_var_read_GBs": read / (t_nv["ms_median"] * 1e-3) / 1e9,
        "copy_read_GBs": read / (t_cp["ms_median"] * 1e-3) / 1e9,
        "em": t_em, "em_noise": t_en,
        "em_ms_per_iter": t_em["ms_median"] / a.iters,
        "em_noise_ms_per_iter": t_en["ms_median"] / a.iters,
        "sigma2_theta0_mean": float(s2.mean()), "sigma2_em_mean": float(s2_em.mean()),
        "sigma2_em_median": float(np.median(s2_em)),
        "nmse_em_mean": nmse_em, "nmse_em_noise_mean": nmse_en,
        "status_any": int(eng.status.max().item()),
    }), flush=True)


if __name__ == "__main__":
    main()
