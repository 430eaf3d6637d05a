#!/usr/bin/env python3
"""NMSE vs SNR with the noise parameter known, wrongly assumed and estimated (sbce_em_noise), on
the data of "Proposed method/SNR/all_Detectors.py" (constants :331-354, generation :362-370)."""
import argparse

from _cli import init_distributed, package, report  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--SNR", type=float, nargs="+", default=[-5, 0, 5, 10, 15, 20])
    ap.add_argument("--T-d", type=int, default=50)
    ap.add_argument("--T-p", type=int, default=12)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--n-rx", type=int, default=2)
    ap.add_argument("--n-tx", type=int, default=2)
    ap.add_argument("--itera", type=int, default=8)
    ap.add_argument("--monte-iter", type=int, default=15)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--varn-assumed", type=float, default=1.0,
                    help="the fixed wrong parameter, and the start of the estimated one")
    ap.add_argument("--power", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", default="soft")
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    init_distributed()
    pkg = package()
    x, curves, ratio = pkg.sweeps.noise_est_vs_snr(
        tuple(a.SNR), a.T_d, a.T_p, a.N, a.n_rx, a.n_tx, a.itera, a.monte_iter, a.M,
        varn_assumed=a.varn_assumed, power=a.power, seed=a.seed, replay=not a.no_replay,
        mode=a.mode)
    cols = {"varn known": curves["known"], f"varn = {a.varn_assumed:g}": curves["assumed"],
            "varn estimated": curves["estimated"], "sigma2_hat/true": ratio}
    report("SNR", x, cols, a.out, "EM with known, assumed and estimated noise variance")


if __name__ == "__main__":
    main()
