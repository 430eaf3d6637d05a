#!/usr/bin/env python3
"""Time sbce_detect (csrc/detect.hip) with HIP events at the cfg1 shape (4x4, P = 65, T_d = 256,
16-QAM, J = 65,536, B = 1000) and at the cfg5 grid's largest point (2x2, P = 16, T_d = 120,
64-QAM, J = 4096, B = 2000), every output enabled; beside it, for scale, one existing sbce_estep
SOFT call on the same buffers.  Warm-up calls first, then --reps timed calls each; prints one JSON
line per shape with median, min and max (the spread) and hypotheses per second.

Usage: python tools/detect_bench.py [--reps 10] [--warmup 2] [--shapes cfg1 cfg5]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

# name: (n_tx, n_rx, P, T_d, M, B)
SHAPES = {"cfg1": (4, 4, 65, 256, 16, 1000), "cfg5": (2, 2, 16, 120, 64, 2000)}
VARN = 0.1


def make_batch(pkg, n_tx, n_rx, P, T_d, M, B, seed=0):
    r = np.random.RandomState(seed)
    cons = pkg.qam.qam_constellation(M)
    K = P * n_tx * n_rx
    nb = min(B, 50)                                   # distinct trials, tiled to the batch
    h = (r.randn(nb, K) + 1j * r.randn(nb, K)) / np.sqrt(2)
    theta = h + 0.05 * (r.randn(nb, K) + 1j * r.randn(nb, K)) / np.sqrt(2)
    psi = np.exp(2j * np.pi * r.uniform(size=(nb, T_d, P)))
    psi[:, :, 0] = 1.0
    x = cons[r.randint(0, M, size=(nb, T_d, n_tx))]
    H = np.einsum("btp,bpar->btra", psi, h.reshape(nb, P, n_tx, n_rx))
    y = np.einsum("btra,bta->btr", H, x)
    y = y + np.sqrt(VARN / 2) * (r.randn(*y.shape) + 1j * r.randn(*y.shape))
    rep = (B + nb - 1) // nb

    def tile(v):
        return np.ascontiguousarray(np.tile(v, (rep,) + (1,) * (v.ndim - 1))[:B])

    return dict(y_d=tile(y), psi_d=tile(psi), theta0=tile(theta), x=tile(x), cons=cons,
                y_p=np.zeros((B, 1, n_rx), complex), u_p=np.zeros((B, 1, P * n_tx), complex))


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
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.load()
    for name in a.shapes:
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
        dims = L.DetectDims(B, n_tx, n_rx, P, T_d, M, 0, VARN * VARN)
        ptrs = L.DetectPtrs(eng.y_d.data_ptr(), eng.psi_d.data_ptr(), eng.cons.data_ptr(),
                            eng.theta.data_ptr(), lab.data_ptr(), None, eng.x_d.data_ptr(),
                            xhat.data_ptr(), idx.data_ptr(), post.data_ptr(), llr.data_ptr(),
                            err.data_ptr(), None, 0)
        stream = torch.cuda.current_stream().cuda_stream

        def detect():
            L.check(lib.sbce_detect(ctypes.byref(dims), ctypes.byref(ptrs), stream), "sbce_detect")

        J = M ** n_tx
        td = timed(torch, detect, a.warmup, a.reps)
        te = timed(torch, eng.estep, a.warmup, a.reps)
        e = err.cpu().numpy()
        print(json.dumps({
            "shape": name, "n_tx": n_tx, "n_rx": n_rx, "P": P, "T_d": T_d, "M": M, "J": J,
            "batch": B, "reps": a.reps, "warmup": a.warmup, "detect": td,
            "hypotheses_per_s": B * T_d * J / (td["ms_median"] * 1e-3),
            "estep_soft": te, "ser": float(e[:, 0].sum() / (B * T_d * n_tx)),
            "ber": float(e[:, 1].sum() / (B * T_d * n_tx * lgM)),
            "finite": bool(torch.isfinite(llr).all().item() and torch.isfinite(post).all().item()),
        }), flush=True)


if __name__ == "__main__":
    main()
