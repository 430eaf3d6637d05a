#!/usr/bin/env python3
"""Time the soft-in / soft-out decoder (csrc/siso.hip) with HIP events: B = 1000 codewords of 800
coded bits -- one 4x4, 16-QAM, T_d = 50 trial each -- for the (133, 171) and the (7, 5) code,
terminated, log-MAP and max-log, with the interleaver; in the same run
  * the A/B arm of the kernel with ONE wave per codeword group (alpha over every step, then beta
    with the outputs) in place of the two-wave split -- both arms in the A/B library, same bits;
  * the sbce_detect_linear_prior call (EP, 5 passes) of the matching batch, whose llr the decoder
    reads: which block bounds an outer iteration of the turbo loop;
  * a device-to-device copy of the decoder's workspace bytes: the bandwidth yardstick of the
    alpha / beta rows it writes once and reads once.
Warm-up calls first, then --reps timed calls each; prints one JSON line with median, min and max.

Usage: python tools/siso_bench.py [--reps 20] [--warmup 3] [--batch 1000]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

N_TX, N_RX, N_RIS, T_P, T_D, M = 4, 4, 4, 24, 50, 16
CODES = {"133_171": ((0o133, 0o171), 7), "7_5": ((0o7, 0o5), 3)}


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1000)
    a = ap.parse_args()
    import torch
    pkg = entry.package()
    L = pkg._lib
    lib = L.use_ab()                                   # both arms from one library
    lib.sbce_debug_siso_onewave.restype = ctypes.c_int
    lib.sbce_debug_siso_onewave.argtypes = [ctypes.c_int]
    em = sys.modules[pkg.__name__ + ".em"]
    B = a.batch
    stream = torch.cuda.current_stream().cuda_stream
    varn = float(pkg.signal_model.snr_to_varn(15.0, 10.0))
    b = pkg.signal_model.synthetic_batch(B, N_TX, N_RX, N_RIS, T_P, T_D, M, varn, seed=0)
    labels = pkg.qam.gray_labeling(M)
    idx = np.argmin(np.abs(b["x_d"][..., None] - b["cons"]), axis=-1)
    la = pkg.qam.prior_llr_gaussian(pkg.qam.bits_of(labels)[idx], 0.5, np.random.default_rng(1))
    dev = [torch.from_numpy(np.ascontiguousarray(b[k])).cuda()
           for k in ("y_d", "psi_d", "cons", "h")]
    lab_d = torch.from_numpy(labels).cuda()
    la_d = torch.from_numpy(la).cuda()
    es = float(np.mean(np.abs(b["cons"]) ** 2))

    def detect():
        return em._detect_linear_call(torch, *dev, N_TX, "ep", varn, None, es, lab_d, None, False,
                                      ("llr",), 5, la=la_d)

    llr = detect()["llr"].reshape(B, -1).contiguous()
    nc = llr.shape[1]
    out = {"batch": B, "coded_bits": nc, "reps": a.reps, "warmup": a.warmup,
           "detect_linear_prior_ep5": timed(torch, detect, a.warmup, a.reps)}
    for name, (gens, K) in CODES.items():
        code = pkg.ConvCode(gens, K, True)
        n_info = code.n_info_for(nc)
        perm = torch.from_numpy(pkg.random_interleaver(nc, 3)).cuda()
        res, bits = {"n_info": n_info, "n_steps": code.n_steps(n_info)}, {}
        for maxlog in (False, True):
            flags = L.SBCE_SISO_TERMINATED | (L.SBCE_DETECT_MAXLOG if maxlog else 0)
            dims = L.SisoDims(B, n_info, K, 2, (ctypes.c_int32 * 3)(*gens, 0), flags)
            nb = ctypes.c_size_t(0)
            L.check(lib.sbce_siso_workspace_bytes(dims, ctypes.byref(nb)), "bytes")
            ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
            le = torch.empty((B, nc), dtype=torch.float64, device="cuda")
            lapp = torch.empty((B, n_info), dtype=torch.float64, device="cuda")
            uhat = torch.empty((B, n_info), dtype=torch.int32, device="cuda")
            ptrs = L.SisoPtrs(llr.data_ptr(), None, perm.data_ptr(), None, lapp.data_ptr(),
                              uhat.data_ptr(), le.data_ptr(), None, ws.data_ptr(), nb.value)

            def decode():
                L.check(lib.sbce_siso_decode(dims, ptrs, stream), "sbce_siso_decode")

            key = "maxlog" if maxlog else "logmap"
            for arm, on in (("two_wave", 0), ("one_wave", 1), ("two_wave_again", 0)):
                lib.sbce_debug_siso_onewave(on)
                res[f"{key}_{arm}"] = timed(torch, decode, a.warmup, a.reps)
                bits[key, arm] = (le.cpu().numpy().copy(), lapp.cpu().numpy().copy())
            lib.sbce_debug_siso_onewave(0)
            res[f"{key}_same_bits"] = bool(all(
                np.array_equal(x, y, equal_nan=True)
                for x, y in zip(bits[key, "two_wave"], bits[key, "one_wave"])))
            if not maxlog:
                res["workspace_bytes"] = nb.value
                dst = torch.empty_like(ws)
                res["d2d_copy_workspace_bytes"] = timed(torch, lambda: dst.copy_(ws), a.warmup,
                                                        a.reps)
                del dst
            del ws
        out[name] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
