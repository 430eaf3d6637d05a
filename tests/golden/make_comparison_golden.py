"""Generate the fixtures of the comparison experiment (proposed EM beside the semi-blind
Gaussian-approximation EM) by running the REFERENCE's own functions in the CPU container:

  comparison_td.npz  "Comparision/Comparision T_d vs NMSE.py" constants, T_d in {20, 100}
  comparison_tp.npz  "Comparision/Comparision T_p .py" constants, T_p in {4, 40}
  approx_small.npz   EM_approx on odd shapes (every boundary of csrc/approx.hip)

Test infrastructure, as make_golden.py (whose ``load_defs`` loads only the import / def
statements of a reference script): never run on the GPU box, only the .npz files travel.
Each sweep fixture follows its script's draw order after ``np.random.seed(0)`` for one trial.

Usage:  python tests/golden/make_comparison_golden.py [td] [tp] [small]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, load_defs, quiet  # noqa: E402

CMP = os.path.join(REF, "Comparision")
TD_SCRIPT = os.path.join(CMP, "Comparision T_d vs NMSE.py")
TP_SCRIPT = os.path.join(CMP, "Comparision T_p .py")

N, N_RX, N_TX, M_SYM, VARN, VARH = 32, 8, 1, 4, 0.1, 1.0
GLOBS = dict(n_tx=N_TX, beta_min=0, beta_max=2 * np.pi)

# (N, M, T_p, T_d, Iterations, varn)
SMALL = [(6, 2, 4, 9, 3, 0.1), (8, 3, 5, 12, 4, 0.3), (33, 5, 7, 65, 6, 0.1),
         (64, 8, 16, 130, 5, 0.1), (17, 1, 3, 40, 5, 0.2), (32, 8, 16, 20, 20, 1.0)]


def _nmse_th(ns, theta, h):
    e = theta - h[:, np.newaxis]
    return float(np.matrix.trace(np.abs(np.matmul(np.conjugate(e).T, e)))
                 / np.power(np.linalg.norm(h[:, np.newaxis]), 2))


def _nmse_g(Gc, G):
    return float(np.matrix.trace(np.abs(np.matmul(np.conjugate(Gc - G).T, Gc - G)))
                 / np.power(np.linalg.norm(G), 2))


def _point(ns, out, tag, T_p, T_d, itera, h, F_H, G, h_prop, X_p, X_d, aps, Ptp, Ptd):
    """One sweep point after the script's symbol / phase draws: both received signals, both EMs."""
    x_p, x_d = np.vstack(X_p), np.vstack(X_d)
    Y_p, Y_d, Z_p, Z_d, h_init = ns["received_proposed"](T_p, T_d, Ptp, Ptd, N_RX, N_TX, X_d, X_p,
                                                         h_prop, VARN, M_SYM)
    z_p, z_d = ns["noise_approx"](VARN, N_RX, T_p, T_d)
    Y_p_dft, Y_d_dft = ns["received_approx"](h, F_H, Ptp, Ptd, x_d, x_p, z_p, z_d)
    theta = quiet(ns["em_proposed"], Y_d, Y_p, T_d, T_p, Z_p, Ptd, aps, M_SYM, VARN, itera, h_init)
    Gc = quiet(ns["EM_approx"], Ptp, Ptd, x_p, Y_p_dft, Y_d_dft, itera, VARN, G)
    S_p = np.matmul(Ptp, np.diagflat(x_p))
    G0 = np.conjugate(np.matmul(Y_p_dft, np.linalg.pinv(S_p))).T
    # the list pinv makes h_initial (T_p, K, 1); the first M-step returns theta to (K, 1)
    theta = np.asarray(theta)
    assert theta.shape == (h_prop.size, 1), theta.shape
    out.update({
        f"{tag}_Psi_p": Ptp, f"{tag}_Psi_d": Ptd, f"{tag}_x_p": x_p, f"{tag}_x_d": x_d,
        f"{tag}_Y_p": np.stack([y[:, 0] for y in Y_p]), f"{tag}_Y_d": np.stack([y[:, 0] for y in Y_d]),
        f"{tag}_h_init": np.asarray(h_init)[:, :, 0],
        f"{tag}_Y_p_dft": Y_p_dft, f"{tag}_Y_d_dft": Y_d_dft, f"{tag}_G0": G0,
        f"{tag}_theta": theta[:, 0], f"{tag}_G_hat": Gc,
        f"{tag}_nmse_proposed": _nmse_th(ns, theta, h_prop), f"{tag}_nmse_approx": _nmse_g(Gc, G),
    })


def make_td(points=(20, 100), T_p=16, itera=20, seed=0):
    ns = load_defs(TD_SCRIPT, **GLOBS)
    np.random.seed(seed)
    h, F_H, G, h_prop = ns["channelMatrix1"](VARH, N, N_RX, N_TX, N_RX, N_TX)
    X_p = ns["pilotSymbols"](N_TX, M_SYM, T_p)
    out = dict(T_d=np.asarray(points), T_p=T_p, N=N, n_rx=N_RX, itera=itera, varn=VARN, seed=seed,
               h=h, F_H=F_H, G=G, h_proposed=h_prop)
    for td in points:
        Ptp, Ptd = ns["irsMatrix"](T_p, td, N, 0, 1)
        X_d, aps = ns["symbols"](N_TX, M_SYM, td)
        _point(ns, out, f"td{td}", T_p, td, itera, h, F_H, G, h_prop, X_p, X_d, aps, Ptp, Ptd)
    np.savez(os.path.join(OUT, "comparison_td.npz"), **out)


def make_tp(points=(4, 40), T_d=50, itera=15, seed=0):
    ns = load_defs(TP_SCRIPT, **GLOBS)
    np.random.seed(seed)
    h, F_H, G, h_prop = ns["channelMatrix1"](VARH, N, N_RX, N_TX, N_RX, N_TX)
    X_d, aps = ns["symbols"](N_TX, M_SYM, T_d)
    out = dict(T_p=np.asarray(points), T_d=T_d, N=N, n_rx=N_RX, itera=itera, varn=VARN, seed=seed,
               h=h, F_H=F_H, G=G, h_proposed=h_prop)
    for tp in points:
        Ptp, Ptd = ns["irsMatrix"](tp, T_d, N, 0, 1)
        X_p = ns["pilotSymbols"](N_TX, M_SYM, tp)
        _point(ns, out, f"tp{tp}", tp, T_d, itera, h, F_H, G, h_prop, X_p, X_d, aps, Ptp, Ptd)
    np.savez(os.path.join(OUT, "comparison_tp.npz"), **out)


def small_case(ns, n, m, tp, td, iters, varn, seed):
    """Inputs of one EM_approx trial from the T_d script's own generators."""
    np.random.seed(seed)
    h, F_H, G, _ = ns["channelMatrix1"](VARH, n, m, 1, m, 1)
    X_p = ns["pilotSymbols"](1, M_SYM, tp)
    Ptp, Ptd = ns["irsMatrix"](tp, td, n, 0, 1)
    X_d, _ = ns["symbols"](1, M_SYM, td)
    x_p, x_d = np.vstack(X_p), np.vstack(X_d)
    z_p, z_d = ns["noise_approx"](varn, m, tp, td)
    Y_p, Y_d = ns["received_approx"](h, F_H, Ptp, Ptd, x_d, x_p, z_p, z_d)
    G0 = np.conjugate(np.matmul(Y_p, np.linalg.pinv(np.matmul(Ptp, np.diagflat(x_p))))).T
    return dict(Psi_p=Ptp, Psi_d=Ptd, x_p=x_p, Y_p=Y_p, Y_d=Y_d, G=G, G0=G0)


def make_small():
    ns = load_defs(TD_SCRIPT, **GLOBS)
    out = dict(shapes=np.asarray(SMALL))
    for k, (n, m, tp, td, iters, varn) in enumerate(SMALL):
        c = small_case(ns, n, m, tp, td, iters, varn, seed=100 + k)
        c["G_hat"] = quiet(ns["EM_approx"], c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"],
                           iters, varn, c["G"])
        out.update({f"c{k}_{name}": v for name, v in c.items()})
    # batch-independence test: the (6, 2, 4, 9) shape with three different seeds (inputs only)
    for s in range(3):
        c = small_case(ns, 6, 2, 4, 9, 3, 0.1, seed=200 + s)
        out.update({f"s{s}_{name}": v for name, v in c.items()})
    np.savez(os.path.join(OUT, "approx_small.npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "td", "tp"]
    for w in which:
        {"td": make_td, "tp": make_tp, "small": make_small}[w]()
        print("wrote", w)
