#!/usr/bin/env python3
"""The code-aided (turbo) loop on the MI355X against SNR: bit error rate of the decoder's decisions
and NMSE of the channel estimate after each outer iteration of em.turbo_em_batch (EM with the
decoder's extrinsic L-values as the prior, soft-input EP detection, BCJR decoding), beside the
genie Cramer-Rao bound of crb_batch -- the estimate the loop would reach with every data symbol
known.  One codeword of the chosen code spans each trial's T_d n_tx log2 M bits, interleaved."""
import argparse

import numpy as np

from _cli import package, report  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--SNR", type=float, nargs="+", default=[6.0, 8.0, 10.0, 12.0, 14.0])
    ap.add_argument("--T-d", type=int, default=50)
    ap.add_argument("--T-p", type=int, default=24)
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--n-rx", type=int, default=4)
    ap.add_argument("--n-tx", type=int, default=4)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--outer", type=int, default=4)
    ap.add_argument("--itera", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--generators", type=lambda s: int(s, 8), nargs="+", default=[0o133, 0o171],
                    help="octal generators, 2 or 3")
    ap.add_argument("--K", type=int, default=7)
    ap.add_argument("--unterminated", action="store_true")
    ap.add_argument("--monte-iter", type=int, default=200)
    ap.add_argument("--power", type=float, default=10.0)
    ap.add_argument("--noise", choices=["em", "true"], default="true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = package()
    q, sm = pkg.qam, pkg.signal_model
    code = pkg.ConvCode(a.generators, a.K, not a.unterminated)
    lgM = int(a.M - 1).bit_length()
    nc = a.T_d * a.n_tx * lgM
    n_info = code.n_info_for(nc)
    rng = np.random.default_rng(a.seed)
    u = rng.integers(0, 2, (a.monte_iter, n_info))
    perm = pkg.random_interleaver(nc, a.seed)
    sent = np.empty((a.monte_iter, nc), dtype=np.int8)
    sent[:, perm] = code.encode(u)
    cons, labels = q.qam_constellation(a.M), q.gray_labeling(a.M)
    x_d = q.map_bits(sent.reshape(a.monte_iter, a.T_d, a.n_tx, lgM), cons, labels)
    ber = {f"BER outer {k + 1}": [] for k in range(a.outer)}
    nm = {f"NMSE outer {k + 1}": [] for k in range(a.outer)}
    nm["CRB genie"] = []
    for snr in a.SNR:
        varn = float(sm.snr_to_varn(snr, a.power))
        b = sm.synthetic_batch(a.monte_iter, a.n_tx, a.n_rx, a.N, a.T_p, a.T_d, a.M, varn,
                               seed=a.seed, x_d=x_d)
        args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"])
        res = pkg.turbo_em_batch(*args, varn, b["theta0"], a.n_tx, code, perm, outer=a.outer,
                                 itera=a.itera, ep_passes=a.passes, labels=labels, noise=a.noise,
                                 u_true=u, h_true=b["h"])
        for k, r in enumerate(res):
            ber[f"BER outer {k + 1}"].append(float(r["bit_errors"].sum()) / u.size)
            nm[f"NMSE outer {k + 1}"].append(float(r["nmse"].mean()))
        nm["CRB genie"].append(float(pkg.crb_batch(*args, a.n_tx, varn, kind="genie", x_d_true=x_d,
                                                   h_true=b["h"], want=("bound",))["bound"].mean()))
    report("SNR", a.SNR, {k: np.array(v) for k, v in ber.items()}, a.out,
           f"turbo loop, K = {a.K} code, {n_info} information bits", ylabel="BER")
    out = None if a.out is None else a.out.replace(".npz", "") + "_nmse.npz"
    report("SNR", a.SNR, {k: np.array(v) for k, v in nm.items()}, out,
           "code-aided EM per outer iteration and the genie bound")


if __name__ == "__main__":
    main()
