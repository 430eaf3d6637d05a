#!/usr/bin/env python3
"""Time the log-likelihood readout and the convergence stop (csrc/loglik.hip) with HIP events:
  (a) one sbce_loglik call (both launches, ll and ll_sym written) against one sbce_detect call
      with every output enabled, on the same buffers in the same process, at the cfg1 shape (4x4,
      P = 65, T_d = 256, 16-QAM, J = 65,536, B = 1000) and at the cfg5 grid's largest point (2x2,
      P = 16, T_d = 120, 64-QAM, J = 4096, B = 2000): tools/detect_bench.py's data;
  (b) sbce_em_conv with min_iters = iters (no stop possible) and no ll_hist against sbce_em at the
      same count, cfg1 shape (tools/noise_bench.py's data at 20 dB), --iters iterations each: the
      difference is the stop's overhead; and the same call with ll_hist, whose difference is the
      cost of the per-iteration log-likelihood.
Warm-up calls first, then --reps timed calls each; prints one JSON line per measurement with
median, min and max.

Usage: python tools/loglik_bench.py [--reps 10] [--warmup 2] [--iters 5 20] [--parts a b]"""
import argparse
import ctypes
import json

import numpy as np

from detect_bench import SHAPES, VARN, entry, make_batch, timed
import noise_bench as nb


def part_a(torch, pkg, a):
    L = pkg._lib
    lib = L.load()
    for name in SHAPES:
        n_tx, n_rx, P, T_d, M, B = SHAPES[name]
        lgM = int(M - 1).bit_length()
        b = make_batch(pkg, n_tx, n_rx, P, T_d, M, B)
        eng = pkg.EMEngine(b, VARN, mode="soft", x_d_true=b["x"])
        lab = torch.from_numpy(pkg.qam.gray_labeling(M)).cuda()
        xhat = torch.empty((B, T_d, n_tx), dtype=torch.complex128, device="cuda")
        idx = torch.empty((B, T_d, n_tx), dtype=torch.int32, device="cuda")
        post = torch.empty((B, T_d, n_tx, M), dtype=torch.float64, device="cuda")
        llr = torch.empty((B, T_d, n_tx, lgM), dtype=torch.float64, device="cuda")
        err = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        ddims = L.DetectDims(B, n_tx, n_rx, P, T_d, M, 0, VARN * VARN)
        dptrs = L.DetectPtrs(eng.y_d.data_ptr(), eng.psi_d.data_ptr(), eng.cons.data_ptr(),
                             eng.theta.data_ptr(), lab.data_ptr(), None, eng.x_d.data_ptr(),
                             xhat.data_ptr(), idx.data_ptr(), post.data_ptr(), llr.data_ptr(),
                             err.data_ptr(), None, 0)
        n = ctypes.c_size_t(0)
        L.check(lib.sbce_loglik_workspace_bytes(ctypes.byref(eng.dims), ctypes.byref(n)), "bytes")
        scratch = torch.empty(max(n.value, 16), dtype=torch.uint8, device="cuda")
        ll = torch.zeros(B, dtype=torch.float64, device="cuda")
        sym = torch.zeros((B, T_d), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def detect():
            L.check(lib.sbce_detect(ctypes.byref(ddims), ctypes.byref(dptrs), stream), "sbce_detect")

        def loglik():
            L.check(lib.sbce_loglik(eng.dims, eng.ptrs, ll.data_ptr(), sym.data_ptr(),
                                    scratch.data_ptr(), scratch.numel(), stream), "sbce_loglik")

        J = M ** n_tx
        tl = timed(torch, loglik, a.warmup, a.reps)
        td = timed(torch, detect, a.warmup, a.reps)
        tl2 = timed(torch, loglik, 0, a.reps)             # again after detect: the order's effect
        print(json.dumps({
            "part": "a", "shape": name, "n_tx": n_tx, "n_rx": n_rx, "P": P, "T_d": T_d, "M": M,
            "J": J, "batch": B, "reps": a.reps, "warmup": a.warmup, "varn": VARN,
            "loglik": tl, "detect_all_outputs": td, "loglik_after_detect": tl2,
            "loglik_over_detect": tl["ms_median"] / td["ms_median"],
            "hypotheses_per_s": B * T_d * J / (tl["ms_median"] * 1e-3),
            "ll_mean": float(ll.mean().item()), "finite": bool(torch.isfinite(sym).all().item()),
        }), flush=True)
        del eng, post, llr


def part_b(torch, pkg, a):
    L = pkg._lib
    lib = L.load()
    B = a.batch
    varn = float(pkg.signal_model.snr_to_varn(20.0))
    batch = pkg.signal_model.synthetic_batch(B, nb.N_TX, nb.N_RX, nb.N_RIS, nb.T_P, nb.T_D, nb.M,
                                             varn, seed=0)
    eng = pkg.EMEngine(batch, varn, mode="soft")
    del batch
    stream = torch.cuda.current_stream().cuda_stream
    n = ctypes.c_size_t(0)
    L.check(lib.sbce_conv_workspace_bytes(ctypes.byref(eng.dims), 1, ctypes.byref(n)), "bytes")
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    for iters in a.iters:
        dth = torch.zeros((B, iters), dtype=torch.float64, device="cuda")
        llh = torch.zeros((B, iters), dtype=torch.float64, device="cuda")
        cv = L.ConvOpts(1e-6, 0.0, iters, 0, dth.data_ptr(), None, scratch.data_ptr(),
                        scratch.numel())
        cvl = L.ConvOpts(1e-6, 0.0, iters, 0, dth.data_ptr(), llh.data_ptr(), scratch.data_ptr(),
                         scratch.numel())

        def em():
            eng.theta.copy_(eng.theta0)
            L.check(lib.sbce_em(eng.dims, eng.ptrs, iters, eng.mode, eng.solve, stream), "sbce_em")

        def conv(opts):
            eng.theta.copy_(eng.theta0)
            L.check(lib.sbce_em_conv(eng.dims, eng.ptrs, iters, eng.mode, eng.solve, None,
                                     ctypes.byref(opts), stream), "sbce_em_conv")

        t_em = timed(torch, em, a.warmup, a.reps)
        th_em = eng.theta.clone()
        t_cv = timed(torch, lambda: conv(cv), a.warmup, a.reps)
        same = bool(torch.equal(th_em, eng.theta))
        t_ll = timed(torch, lambda: conv(cvl), a.warmup, a.reps)
        t_em2 = timed(torch, em, 0, a.reps)               # again: the spread between repeats
        print(json.dumps({
            "part": "b", "shape": "cfg1", "batch": B, "iters": iters, "reps": a.reps,
            "warmup": a.warmup, "varn_true": varn, "em": t_em, "em_again": t_em2,
            "em_conv_no_stop": t_cv, "em_conv_ll_hist": t_ll,
            "stop_overhead_ms_per_iter": (t_cv["ms_median"] - t_em["ms_median"]) / iters,
            "ll_hist_ms_per_iter": (t_ll["ms_median"] - t_cv["ms_median"]) / iters,
            "em_ms_per_iter": t_em["ms_median"] / iters, "theta_bitwise_equal": same,
            "dtheta_last_median": float(dth[:, -1].median().item()),
            "ll_monotone_frac": float((llh[:, 1:] >= llh[:, :-1] - 1e-9 * llh[:, 1:].abs())
                                      .all(dim=1).double().mean().item()),
        }), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--parts", nargs="+", default=["a", "b"], choices=["a", "b"])
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    if "a" in a.parts:
        part_a(torch, pkg, a)
    if "b" in a.parts:
        part_b(torch, pkg, a)


if __name__ == "__main__":
    main()
