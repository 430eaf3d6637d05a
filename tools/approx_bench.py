#!/usr/bin/env python3
"""Time sbce_approx_em (csrc/approx.hip) at the T_d comparison script's largest point: N = 32,
M = 8, T_p = 16, T_d = 100, 21 updates, for batches of 256, 1024 and 4096 trials, with HIP
events after a warm-up; and the NumPy restatement (tests/approx_oracle.py) on the host for 8
trials.  Prints one JSON line per batch: median, min and max over the repetitions.

Usage: python tools/approx_bench.py [--reps 20] [--batches 256 1024 4096] [--once B]
(--once B: one warm call and one timed call at batch B, for a kernel trace)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

N, M, T_P, T_D, UPDATES, VARN = 32, 8, 16, 100, 21, 0.1


def make_batch(sm, B, seed=0):
    """B trials from the package's generators (per-trial RandomState, the scripts' draw order)."""
    out = {k: [] for k in ("y_d", "y_p", "psi_d", "psi_p", "x_p", "g0")}
    for i in range(B):
        rs = np.random.RandomState(seed * 100003 + i)
        h, F_H, G, _ = sm.channel_matrix1(1.0, N, M, 1, rs=rs)
        x_p = np.vstack(sm.pilot_symbols(1, 4, T_P, rs=rs))
        Ptp, Ptd = sm.irs_matrix_nodirect(T_P, T_D, N, rs=rs)
        x_d = np.vstack(sm.symbols(1, 4, T_D, rs=rs)[0])
        z_p, z_d = sm.noise_approx(VARN, M, T_P, T_D, rs=rs)
        Y_p = (F_H @ (Ptp * h)) * x_p.T + z_p
        Y_d = (F_H @ (Ptd * h)) * x_d.T + z_d
        for k, v in zip(out, (Y_d.T, Y_p.T, Ptd.T, Ptp.T, x_p.reshape(-1),
                              sm.initial_g_approx(Ptp, x_p, Y_p))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    base = make_batch(pkg.signal_model, 64)
    stream = torch.cuda.current_stream().cuda_stream
    for B in ([a.once] if a.once else a.batches):
        t = {k: torch.from_numpy(np.ascontiguousarray(np.tile(v, (B // 64 + 1,) + (1,) * (v.ndim - 1))[:B])).cuda()
             for k, v in base.items()}
        g = t["g0"].clone()
        status = torch.zeros(B, dtype=torch.int32, device="cuda")
        dims = L.ApproxDims(B, N, M, T_P, T_D, 0, VARN)
        ptrs = L.ApproxPtrs(t["y_d"].data_ptr(), t["y_p"].data_ptr(), t["psi_d"].data_ptr(),
                            t["psi_p"].data_ptr(), t["x_p"].data_ptr(), g.data_ptr(), None,
                            status.data_ptr(), None, 0)

        def call():
            g.copy_(t["g0"])
            L.check(lib.sbce_approx_em(ctypes.byref(dims), ctypes.byref(ptrs), UPDATES, stream),
                    "sbce_approx_em")

        call()
        torch.cuda.synchronize()
        if a.once:
            call()
            torch.cuda.synchronize()
            print(json.dumps({"batch": B, "status_nonzero": int((status != 0).sum())}))
            return
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g.copy_(t["g0"])
            e0.record()
            L.check(lib.sbce_approx_em(ctypes.byref(dims), ctypes.byref(ptrs), UPDATES, stream),
                    "sbce_approx_em")
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.asarray(ms)
        print(json.dumps({"batch": B, "updates": UPDATES, "reps": a.reps,
                          "ms_median": float(np.median(ms)), "ms_min": float(ms.min()),
                          "ms_max": float(ms.max()),
                          "trial_updates_per_s": B * UPDATES / (float(np.median(ms)) * 1e-3),
                          "status_nonzero": int((status != 0).sum())}), flush=True)
    import approx_oracle as ao
    b8 = {k: v[:8] for k, v in base.items()}
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for i in range(8):
            ao.em_approx(b8["psi_p"][i].T, b8["psi_d"][i].T, b8["x_p"][i], b8["y_p"][i].T,
                         b8["y_d"][i].T, UPDATES, VARN, G0=b8["g0"][i])
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"numpy_restatement_trials": 8, "ms_median": float(np.median(ts)),
                      "ms_min": float(min(ts)), "ms_max": float(max(ts))}))


if __name__ == "__main__":
    main()
