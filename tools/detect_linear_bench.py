#!/usr/bin/env python3
"""Time sbce_detect_linear (csrc/detect_linear.hip) with HIP events at the cfg1 shape (4x4, P = 65,
T_d = 256, 16-QAM, B = 1000) and at 8x8 with the same P, T_d, table and batch; MMSE and ZF, once
with every output and once with the soft outputs a decoder reads (x_soft, nu, llr).  Beside it,
for scale, sbce_detect at the cfg1 shape (the exhaustive detector does not take 8 streams).
Warm-up calls first, then --reps timed calls each; prints one JSON line per (shape, kind, output
set) with median, min and max, the algorithmic bytes of the call and the fraction of the HBM
peak they amount to at the median time.

Usage: python tools/detect_linear_bench.py [--reps 10] [--warmup 2] [--shapes cfg1 8x8]"""
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
from detect_bench import make_batch, timed, VARN  # noqa: E402

# name: (n_tx, n_rx, P, T_d, M, B)
SHAPES = {"cfg1": (4, 4, 65, 256, 16, 1000), "8x8": (8, 8, 65, 256, 16, 1000)}
HBM_PEAK_GBS = 8000.0
OUTPUT_SETS = {"all": ("x_soft", "nu", "x_hat", "idx", "post", "llr", "moments", "status", "err"),
               "soft": ("x_soft", "nu", "llr")}


def algorithmic_bytes(n_tx, n_rx, P, T_d, M, B, outs):
    """Each input read once (theta 16 P NE per trial, psi_d 16 T_d P, y_d 16 T_d n_rx) and each
    requested output written once."""
    lgM = int(M - 1).bit_length()
    per_sym = {"x_soft": 16 * n_tx, "nu": 8 * n_tx, "x_hat": 16 * n_tx, "idx": 4 * n_tx,
               "post": 8 * n_tx * M, "llr": 8 * n_tx * lgM, "moments": 16 * (n_tx + n_tx * n_tx)}
    rd = B * (16 * P * n_tx * n_rx + 16 * T_d * P + 16 * T_d * n_rx)
    if "err" in outs:
        rd += B * T_d * 16 * n_tx                      # x_d_true
    wr = B * T_d * sum(per_sym[k] for k in outs if k in per_sym)
    return rd, wr


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
    stream = torch.cuda.current_stream().cuda_stream
    for name in a.shapes:
        n_tx, n_rx, P, T_d, M, B = SHAPES[name]
        lgM = int(M - 1).bit_length()
        b = make_batch(pkg, n_tx, n_rx, P, T_d, M, B)
        dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda()
               for k in ("y_d", "psi_d", "theta0", "x", "cons")}
        lab = torch.from_numpy(pkg.qam.gray_labeling(M)).cuda()
        c128, f64, i32 = torch.complex128, torch.float64, torch.int32
        buf = {"x_soft": torch.empty((B, T_d, n_tx), dtype=c128, device="cuda"),
               "nu": torch.empty((B, T_d, n_tx), dtype=f64, device="cuda"),
               "x_hat": torch.empty((B, T_d, n_tx), dtype=c128, device="cuda"),
               "idx": torch.empty((B, T_d, n_tx), dtype=i32, device="cuda"),
               "post": torch.empty((B, T_d, n_tx, M), dtype=f64, device="cuda"),
               "llr": torch.empty((B, T_d, n_tx, lgM), dtype=f64, device="cuda"),
               "moments": torch.empty((B, T_d, n_tx + n_tx * n_tx), dtype=c128, device="cuda"),
               "status": torch.empty((B,), dtype=i32, device="cuda"),
               "err": torch.empty((B, 2), dtype=i32, device="cuda")}
        es = float(np.mean(np.abs(b["cons"]) ** 2))
        base = None
        if name == "cfg1":
            dd = L.DetectDims(B, n_tx, n_rx, P, T_d, M, 0, VARN * VARN)
            dp = L.DetectPtrs(dev["y_d"].data_ptr(), dev["psi_d"].data_ptr(), dev["cons"].data_ptr(),
                              dev["theta0"].data_ptr(), lab.data_ptr(), None, dev["x"].data_ptr(),
                              buf["x_hat"].data_ptr(), buf["idx"].data_ptr(), buf["post"].data_ptr(),
                              buf["llr"].data_ptr(), buf["err"].data_ptr(), None, 0)
            base = timed(torch, lambda: L.check(lib.sbce_detect(ctypes.byref(dd), ctypes.byref(dp),
                                                                stream), "sbce_detect"),
                         a.warmup, a.reps)
        for kind in ("mmse", "zf"):
            for oname, outs in OUTPUT_SETS.items():
                dims = L.LinearDims(B, n_tx, n_rx, P, T_d, M,
                                    L.SBCE_LINEAR_MMSE if kind == "mmse" else L.SBCE_LINEAR_ZF, 0,
                                    VARN * VARN, es)

                def ptr(k):
                    return buf[k].data_ptr() if k in outs else None

                ptrs = L.LinearPtrs(y_d=dev["y_d"].data_ptr(), psi_d=dev["psi_d"].data_ptr(),
                                    cons=dev["cons"].data_ptr(), theta=dev["theta0"].data_ptr(),
                                    labels=lab.data_ptr(),
                                    x_d_true=dev["x"].data_ptr() if "err" in outs else None,
                                    x_soft=ptr("x_soft"), nu=ptr("nu"), x_hat=ptr("x_hat"),
                                    idx_hat=ptr("idx"), post=ptr("post"), llr=ptr("llr"),
                                    err=ptr("err"), moments=ptr("moments"), status=ptr("status"))

                def call():
                    L.check(lib.sbce_detect_linear(ctypes.byref(dims), ctypes.byref(ptrs), stream),
                            "sbce_detect_linear")

                t = timed(torch, call, a.warmup, a.reps)
                rd, wr = algorithmic_bytes(n_tx, n_rx, P, T_d, M, B, outs)
                gbs = (rd + wr) / (t["ms_median"] * 1e-3) / 1e9
                line = {"shape": name, "n_tx": n_tx, "n_rx": n_rx, "P": P, "T_d": T_d, "M": M,
                        "batch": B, "kind": kind, "outputs": oname, "reps": a.reps,
                        "warmup": a.warmup, "linear": t, "bytes_read": rd, "bytes_written": wr,
                        "gb_per_s": gbs, "hbm_frac_algorithmic": gbs / HBM_PEAK_GBS,
                        "symbols_per_s": B * T_d / (t["ms_median"] * 1e-3),
                        "finite": bool(torch.isfinite(buf["llr"]).all().item())}
                if "err" in outs:
                    e = buf["err"].cpu().numpy()
                    line["ser"] = float(e[:, 0].sum() / (B * T_d * n_tx))
                    line["status_any"] = bool(buf["status"].any().item())
                if base is not None:
                    line["sbce_detect"] = base
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
