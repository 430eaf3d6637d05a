#!/usr/bin/env python3
"""NMSE vs T_d of the proposed EM beside the semi-blind Gaussian-approximation EM — entry point
of "Comparision/Comparision T_d vs NMSE.py" (constants :203-222, driver :228-253), on the MI355X."""
import argparse

from _cli import init_distributed, package, report  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--T-d", type=int, nargs="+", default=[20, 30, 40, 50, 60, 70, 80, 90, 100])
    ap.add_argument("--T-p", type=int, default=16)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--n-rx", type=int, default=8)
    ap.add_argument("--itera", type=int, default=20)
    ap.add_argument("--monte-iter", type=int, default=1)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--varn", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    init_distributed()
    pkg = package()
    x, curves = pkg.sweeps.comparison_vs_td(tuple(a.T_d), a.T_p, a.N, a.n_rx, a.itera,
                                            a.monte_iter, a.M, a.varn, a.seed,
                                            replay=not a.no_replay)
    report("T_d", x, {"Proposed method": curves["proposed"],
                         "Approximation method": curves["approx"]}, a.out,
           "Comparison between proposed method and the semi-blind Gaussian method")


if __name__ == "__main__":
    main()
