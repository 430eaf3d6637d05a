#!/usr/bin/env python3
"""Uncoded SER / BER vs SNR of the joint ML detector fed each estimator's channel (pilot-only
start, the EM variants, perfect CSI), on the data layout of "Proposed method/SNR/
all_Detectors.py" (:362-370), on the MI355X.  Prints SER, BER and NMSE per estimator."""
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
    ap.add_argument("--itera", type=int, default=5)
    ap.add_argument("--monte-iter", type=int, default=15)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--estimators", nargs="+",
                    default=["pilot", "soft", "hard", "pm", "zf", "mmse", "genie"],
                    help="pilot, genie, or an EM mode: soft hard pm pm_soft zf mmse (n_tx <= 8 "
                         "but soft / hard: <= 4) and the soft mmse_soft zf_soft ep (n_tx <= 8)")
    ap.add_argument("--power", type=float, default=10.0)
    ap.add_argument("--noise", choices=["em", "true"], default="em")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--detector", choices=["ml", "mmse", "zf", "ep"], default="ml",
                    help="joint ML (n_tx <= 4) or per-stream LMMSE / ZF / expectation-propagation "
                         "soft detection (n_tx <= 8)")
    a = ap.parse_args()
    init_distributed()
    pkg = package()
    x, ser, ber, nmse = pkg.sweeps.detection_vs_snr(
        tuple(a.SNR), a.T_d, a.T_p, a.N, a.n_rx, a.n_tx, a.itera, a.monte_iter, a.M,
        tuple(a.estimators), a.power, a.seed, replay=not a.no_replay, noise=a.noise,
        detector=a.detector)
    curves = {f"SER {e}": v for e, v in ser.items()}
    curves.update({f"BER {e}": v for e, v in ber.items()})
    title = {"ml": "ML", "mmse": "LMMSE", "zf": "ZF", "ep": "EP"}[a.detector]
    report("SNR", x, curves, a.out, f"{title} detection per channel estimate", ylabel="error rate",
           logy=True)
    report("SNR", x, {f"NMSE {e}": v for e, v in nmse.items()})


if __name__ == "__main__":
    main()
