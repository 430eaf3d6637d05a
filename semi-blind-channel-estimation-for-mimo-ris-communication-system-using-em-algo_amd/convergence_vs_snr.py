#!/usr/bin/env python3
"""NMSE and iterations performed vs SNR of the EM with a fixed iteration count, with the truth-free
convergence stop (sbce_em_conv) and with the oracle stop on the true channel, on the data of
"Proposed method/SNR/all_Detectors.py" (constants :331-354, generation :362-370)."""
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
    ap.add_argument("--itera", type=int, default=20, help="the fixed count, and the stops' cap")
    ap.add_argument("--monte-iter", type=int, default=15)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--tol-theta", type=float, default=1e-6)
    ap.add_argument("--min-iters", type=int, default=2)
    ap.add_argument("--power", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", default="soft")
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    init_distributed()
    pkg = package()
    x, nmse, its = pkg.sweeps.convergence_vs_snr(
        tuple(a.SNR), a.T_d, a.T_p, a.N, a.n_rx, a.n_tx, a.itera, a.monte_iter, a.M,
        tol_theta=a.tol_theta, min_iters=a.min_iters, power=a.power, seed=a.seed,
        replay=not a.no_replay, mode=a.mode)
    cols = {}
    for arm, label in (("fixed", f"{a.itera} iterations"), ("stop", "truth-free stop"),
                       ("oracle", "oracle stop")):
        cols[f"NMSE {label}"] = nmse[arm]
        cols[f"iters {label}"] = its[arm]
    report("SNR", x, cols, a.out, "EM with a fixed count, the truth-free stop and the oracle stop")


if __name__ == "__main__":
    main()
