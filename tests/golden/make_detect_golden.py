"""Generate tests/golden/detect.npz: the reference modem's labelling and soft-demapper L-values
("Proposed method/QAM.py", loaded as make_golden.py loads it, with the NumPy aliases removed in
NumPy 2 restored) and the inputs of the detector's GPU test shapes.

Test infrastructure: reads the reference tree (read-only) as the oracle of record, is never run on
the GPU box, records data only.

Usage:  python tests/golden/make_detect_golden.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REF = "/root/reference"
PMD = os.path.join(REF, "Proposed method")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

from detect_oracle import detect_ref  # noqa: E402

# (n_tx, n_rx, P, T_d, M, table): the GPU tier's shapes (tests/test_gpu_detect.py)
SHAPES = [(1, 1, 1, 16, 16, "qam"), (2, 2, 5, 12, 4, "qam"), (3, 2, 4, 9, 4, "qam"),
          (4, 4, 3, 7, 16, "qam"), (2, 3, 6, 10, 64, "qam"), (4, 8, 2, 5, 4, "qam"),
          (1, 4, 33, 8, 64, "qam"), (2, 2, 3, 6, 2, "bpsk"), (2, 2, 3, 6, 8, "psk8")]
VARNS = (0.1, 1.0)
B = 3
N0S = (1.0, 0.25)           # the modem's noise density at the two recorded channel_snr values
N_POINTS = 40


def load_qam():
    for name, typ in (("int", int), ("float", float), ("complex", complex)):
        if not hasattr(np, name):
            setattr(np, name, typ)
    spec = importlib.util.spec_from_file_location("ref_qam", os.path.join(PMD, "QAM.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table(kind, M, qam_tables):
    if kind == "qam":
        return qam_tables[M], None
    if kind == "bpsk":
        return np.array([-1.0 + 0j, 1.0 + 0j]), np.arange(2, dtype=np.int32)
    return np.exp(2j * np.pi * np.arange(8) / 8), np.arange(8, dtype=np.int32)   # natural labels


def main():
    qam = load_qam()
    out = {"varns": np.array(VARNS), "n0s": np.array(N0S),
           "shapes": np.array([s[:5] for s in SHAPES], dtype=np.int64),
           "tables": np.array([s[5] for s in SHAPES])}
    qam_tables, labelings = {}, {}
    rs = np.random.RandomState(20240607)
    for M in (4, 16, 64):
        mod = qam.QAModulation(M)
        qam_tables[M] = np.asarray(mod.constellation, dtype=complex)
        labelings[M] = np.asarray(mod.labeling, dtype=np.int32)
        out[f"cons_{M}"] = qam_tables[M]
        out[f"labeling_{M}"] = labelings[M]
        L = int(np.sqrt(M))
        # points inside and just outside the hull, so that no exp() of the naive p0 / p1 underflows
        rx = rs.uniform(-L - 0.5, L + 0.5, N_POINTS) + 1j * rs.uniform(-L - 0.5, L + 0.5, N_POINTS)
        out[f"rx_{M}"] = rx
        for i, n0 in enumerate(N0S):
            mod.channel_snr = mod.energy_per_symbol / n0
            # single far terms may underflow (harmless); p0 / p1 themselves must not
            with np.errstate(divide="raise", invalid="raise", over="raise"):
                lv = np.asarray(mod.demodulate(rx, "soft"), dtype=float)
            assert np.all(np.isfinite(lv)), (M, n0)
            # the reference's own p0, p1 are finite and non-zero: redo its sums to check
            bits = np.array([[(int(l) >> k) & 1 for k in range(mod.bits_per_symbol)]
                             for l in mod.labeling])
            w = np.exp(-np.abs(rx[:, None] - qam_tables[M][None, :]) ** 2 / n0)
            for k in range(mod.bits_per_symbol):
                for v in (0, 1):
                    p = w[:, bits[:, k] == v].sum(axis=1)
                    assert np.all(p > 1e-290) and np.all(np.isfinite(p)), (M, n0, k, v)
            out[f"lvalues_{M}_{i}"] = lv.reshape(N_POINTS, mod.bits_per_symbol)
    min_gap = np.inf
    for si, (n_tx, n_rx, P, T_d, M, kind) in enumerate(SHAPES):
        cons, lab = table(kind, M, qam_tables)
        r = np.random.RandomState(1000 + si)
        K = P * n_tx * n_rx
        h = (r.randn(B, K) + 1j * r.randn(B, K)) / np.sqrt(2)
        theta = h + 0.05 * (r.randn(B, K) + 1j * r.randn(B, K)) / np.sqrt(2)
        psi = np.exp(2j * np.pi * r.uniform(size=(B, T_d, P)))
        psi[:, :, 0] = 1.0                                     # the direct path's row of ones
        xi = r.randint(0, M, size=(B, T_d, n_tx))
        H = np.einsum("btp,bpar->btra", psi, h.reshape(B, P, n_tx, n_rx))
        clean = np.einsum("btra,bta->btr", H, cons[xi])
        z = (r.randn(B, T_d, n_rx) + 1j * r.randn(B, T_d, n_rx)) / np.sqrt(2)
        out[f"s{si}_cons"] = cons
        if lab is not None:
            out[f"s{si}_labels"] = lab
        out[f"s{si}_h"], out[f"s{si}_theta"], out[f"s{si}_psi"] = h, theta, psi
        out[f"s{si}_x"] = cons[xi]
        for vi, varn in enumerate(VARNS):
            y = clean + np.sqrt(varn) * z
            out[f"s{si}_y{vi}"] = y
            # exact decision equality is a fair demand only where the best two distances differ
            for sig2 in (varn ** 2,):
                g = detect_ref(y, psi, cons, theta, sig2, n_tx)["gap"]
                assert g.min() > 1e-6, (si, varn, g.min())
                min_gap = min(min_gap, g.min())
    print("smallest relative gap of the two best distances:", min_gap)
    np.savez_compressed(os.path.join(OUT, "detect.npz"), **out)
    print("wrote detect.npz,", os.path.getsize(os.path.join(OUT, "detect.npz")), "bytes")


if __name__ == "__main__":
    main()
