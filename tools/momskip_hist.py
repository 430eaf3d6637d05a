#!/usr/bin/env python3
"""What the moment-repeat rule skips on bench.py's cfg1 workload (1000 trials,
seed 0), as one JSON line:

* `skipped_by_iters`: the A/B build's counter of skipped trial-M-steps (sbce_debug_momskip) after
  sbce_em(k), k = 1 .. kmax -- the cumulative number of trials the rule froze by iteration k;
* `fixed_point_hist`: sbce_em_conv(tol_theta=0, min_iters=1) iters_done, the iteration after which
  a trial's theta repeats bit for bit;
* `at_fixed_point`: per fixed-point iteration k >= 2, how the moments of the E-step of iteration k
  (sbce_estep on theta_{k-1} of the chained sbce_em(1) calls) compare with those of iteration
  k - 1: `bitwise` equal (the rule skips the M-step), equal as numbers but not in the sign of a
  zero (`zero_sign`), or different in value (`value`: a fixed point the moments do not announce).

  python tools/momskip_hist.py [snr_db] [kmax] > profiles/momfreeze/momskip_hist.json
"""
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-blind-channel-estimation-for-mimo-ris-communication-system-using-em-algo_amd"


def main():
    sbce = importlib.import_module(PKG)
    snr = float(sys.argv[1]) if len(sys.argv) > 1 else 20.0
    kmax = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    trials, iters, n_tx = 1000, 20, 4
    varn = float(sbce.signal_model.snr_to_varn(snr))
    b = sbce.signal_model.synthetic_batch(trials, n_tx, 4, 64, 16, 256, 16, varn, seed=0)
    args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], varn)
    cit = sbce.em_batch_conv(*args, iters, b["theta0"], tol_theta=0.0, min_iters=1)["iters_done"]
    skipped = {}
    with sbce._lib.debug_env() as lib:
        for k in range(1, kmax + 1):
            lib.sbce_debug_momskip(None, 1)
            sbce.em_batch(*args, k, b["theta0"])
            n = ctypes.c_ulonglong(0)
            lib.sbce_debug_momskip(ctypes.byref(n), 0)
            skipped[k] = int(n.value)
    th, prev, cls = b["theta0"], None, {}
    for k in range(1, kmax + 1):                     # E-step of iteration k reads theta_{k-1}
        m, S = sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], th, varn, n_tx)
        mom = np.concatenate([m, S.reshape(trials, S.shape[1], -1)], axis=2)
        if prev is not None:
            sel = cit == k
            bits = np.all(mom.view(np.uint64) == prev.view(np.uint64), axis=(1, 2))
            vals = np.all(mom == prev, axis=(1, 2))
            cls[k] = {"trials": int(sel.sum()), "bitwise": int((sel & bits).sum()),
                      "zero_sign": int((sel & vals & ~bits).sum()),
                      "value": int((sel & ~vals).sum())}
        prev = mom
        th = sbce.em_batch(*args, 1, th)["theta"]
    hist = {int(k): int(v) for k, v in zip(*np.unique(cit, return_counts=True))}
    print(json.dumps({"snr_db": snr, "fixed_point_hist": hist, "skipped_by_iters": skipped,
                      "at_fixed_point": cls}))


if __name__ == "__main__":
    main()
