#!/usr/bin/env python3
"""EXIT chart of the soft-input EP detector on the MI355X: extrinsic information I_E of its bit
L-values against the a-priori information I_A of consistent-Gaussian L-values (qam.
prior_llr_gaussian), for p = 1 pass (the soft-cancellation MMSE turbo detector) and p = 5, from
the true channel and from the channel the code-aided EM estimates with the same a-priori
L-values.  With --nmse: the NMSE of that EM against I_A, beside the pilot-only and the genie
Cramer-Rao bounds of crb_batch -- the two ends the curve runs between (the reference's DFT pilot
phases repeat the direct path's row, so on this data the pilot-only bound is infinite: the
pilots alone do not identify the channel).  With --decoder: the transfer curve of the BCJR decoder
(siso_decode_batch) for one codeword per trial, I_E of its extrinsic coded-bit L-values against
I_A of the L-values it is given."""
import argparse

import numpy as np

from _cli import package, report  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--IA", type=float, nargs="+", default=[0.0, 0.2, 0.4, 0.6, 0.8, 0.95, 1.0])
    ap.add_argument("--SNR", type=float, default=15.0)
    ap.add_argument("--T-d", type=int, default=50)
    ap.add_argument("--T-p", type=int, default=24)
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--n-rx", type=int, default=4)
    ap.add_argument("--n-tx", type=int, default=4)
    ap.add_argument("--itera", type=int, default=5)
    ap.add_argument("--monte-iter", type=int, default=200)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--power", type=float, default=10.0)
    ap.add_argument("--noise", choices=["em", "true"], default="true",
                    help="the detector's sigma^2: the noise the data carry (true) or its square, "
                         "the reference's EM posterior (em)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nmse", action="store_true")
    ap.add_argument("--decoder", action="store_true",
                    help="also the decoder's transfer curve: I_E of siso_decode_batch's le_c "
                         "against I_A of consistent-Gaussian L-values on the coded bits (the curve "
                         "that must fit under the detector's, axes swapped)")
    ap.add_argument("--generators", type=lambda s: int(s, 8), nargs="+", default=[0o133, 0o171],
                    help="--decoder: octal generators, 2 or 3")
    ap.add_argument("--K", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = package()
    q, sm = pkg.qam, pkg.signal_model
    varn = float(sm.snr_to_varn(a.SNR, a.power))
    b = sm.synthetic_batch(a.monte_iter, a.n_tx, a.n_rx, a.N, a.T_p, a.T_d, a.M, varn, seed=a.seed)
    labels = q.gray_labeling(a.M)
    idx = np.argmin(np.abs(b["x_d"][..., None] - b["cons"]), axis=-1)
    bits = q.bits_of(labels)[idx]
    rng = np.random.default_rng(a.seed + 1)
    args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"])
    curves = {f"I_E p={p} {ch}": [] for p in a.passes for ch in ("true h", "EM")}
    nm = {"NMSE EM(ep, prior)": [], "CRB pilot": [], "CRB genie": []}
    crb = {k: pkg.crb_batch(*args, a.n_tx, varn, kind=k, x_d_true=b["x_d"], h_true=b["h"],
                            want=("bound",))["bound"].mean() for k in ("pilot", "genie")}
    # the EM's posterior divides by its parameter squared (the reference's convention): sqrt(varn)
    # makes that the noise the data carry, as the detector's noise="true"
    varn_em = float(np.sqrt(varn)) if a.noise == "true" else varn
    for ia in a.IA:
        la = q.prior_llr_gaussian(bits, ia, rng)
        em = pkg.em_batch(*args, varn_em, a.itera, b["theta0"], mode="ep", prior_llr=la, labels=labels)
        nm["NMSE EM(ep, prior)"].append(float(pkg.nmse_batch(em["theta"], b["h"]).mean().item()))
        nm["CRB pilot"].append(float(crb["pilot"]))
        nm["CRB genie"].append(float(crb["genie"]))
        for p in a.passes:
            for ch, theta in (("true h", b["h"]), ("EM", em["theta"])):
                r = pkg.detect_linear_prior_batch(b["y_d"], b["psi_d"], b["cons"], theta, varn,
                                                  a.n_tx, la, kind=("ep", p), labels=labels,
                                                  noise=a.noise, want=("llr",))
                curves[f"I_E p={p} {ch}"].append(q.bit_mutual_information(r["llr"], bits))
    curves = {k: np.array(v) for k, v in curves.items()}
    report("I_A", a.IA, curves, a.out, "EXIT chart of the soft-input EP detector", ylabel="I_E",
           logy=False)
    if a.nmse:
        out = None if a.out is None else a.out.replace(".npz", "") + "_nmse.npz"
        report("I_A", a.IA, {k: np.array(v) for k, v in nm.items()}, out,
               "code-aided EM between the pilot-only and the genie bound")
    if a.decoder:
        # one codeword per trial, of the length the detector's llr of a trial has
        code = pkg.ConvCode(a.generators, a.K, True)
        nc = a.T_d * a.n_tx * int(a.M - 1).bit_length()
        drng = np.random.default_rng(a.seed + 2)
        c = code.encode(drng.integers(0, 2, (a.monte_iter, code.n_info_for(nc))))
        ie = [q.bit_mutual_information(
            pkg.siso_decode_batch(q.prior_llr_gaussian(c, ia, drng), code, want=("le_c",))["le_c"], c)
            for ia in a.IA]
        out = None if a.out is None else a.out.replace(".npz", "") + "_decoder.npz"
        report("I_A", a.IA, {f"I_E decoder K={a.K}": np.array(ie)}, out,
               "EXIT transfer curve of the decoder", ylabel="I_E", logy=False)


if __name__ == "__main__":
    main()
