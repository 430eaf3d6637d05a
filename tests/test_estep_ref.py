"""CPU tier: the extended-precision E-step restatement (tests/estep_ref.py) against the float64
oracle on square-QAM shapes, its tables against csrc/sbce_internal.h grid_build's classes, and
its tie behaviour (first minimum in product order, uniform posterior)."""
import numpy as np
import pytest

import estep_ref as er
from oracle.em_reduced import estep_moments


@pytest.mark.parametrize("shape", [(2, 2, 4, 9, 16, 10), (3, 4, 3, 7, 4, 0), (2, 3, 2, 5, 64, 25)])
def test_restatement_matches_oracle_on_square_qam(sbce, shape):
    n_tx, n_rx, N, T_d, M, snr = shape
    cons = er.qam(M)
    assert np.array_equal(cons, sbce.qam.qam_constellation(M))
    b = er.synthetic_batch(cons, 2, n_tx, n_rx, N, T_d, snr, seed=3)
    aps = sbce.qam.all_possible_symbols(cons, n_tx)
    scale = np.abs(cons).max() ** 2
    for th in (b["theta_wide"], b["theta_narrow"]):
        ref = er.batch_moments(th, b["y_d"], b["psi_d"], cons, b["varn"], n_tx)
        assert ref["gap"].min() > 1e-9
        for i in range(2):
            m0, S0, _, _ = estep_moments(th[i], b["y_d"][i], b["psi_d"][i].T, aps, b["varn"])
            assert np.abs(ref["m"][i] - m0).max() < 1e-12 * scale
            assert np.abs(ref["S"][i] - S0).max() < 1e-12 * scale
            mh, Sh, _, _ = estep_moments(th[i], b["y_d"][i], b["psi_d"][i].T, aps, b["varn"], "hard")
            assert np.array_equal(ref["mh"][i], mh)
            assert np.abs(ref["Sh"][i] - Sh).max() < 1e-12 * scale


def test_chunking_does_not_change_the_result():
    cons = er.table("psk8")
    b = er.synthetic_batch(cons, 1, 3, 3, 2, 1, 10, seed=5)
    H = er.heff(b["theta_wide"][0], b["psi_d"][0], 3, 3)[0]
    y = b["y_d"][0, 0].astype(er.CLD)
    one = er.symbol_moments(H, y, cons, b["varn"])
    many = er.symbol_moments(H, y, cons, b["varn"], chunk=100)          # 512 = 5 * 100 + 12
    for k in ("m", "S"):
        assert np.abs(one[k] - many[k]).max() < 1e-17
    assert one["jh"] == many["jh"] and one["gap"] == many["gap"]


def test_tables_and_grid_classes():
    """The class grid_build puts each table in: K > 0 (a level grid in any order) or 0."""
    want = {"qam16": 4, "qam64": 8, "qam16_perm": 4, "qam64_perm": 8, "qam16_uneven": 4,
            "qam16_rot": 0, "psk8": 0, "psk16": 0, "bpsk": 0, "cross32": 0, "apsk64": 0}
    size = {"qam16": 16, "qam64": 64, "qam16_perm": 16, "qam64_perm": 64, "qam16_uneven": 16,
            "qam16_rot": 16, "psk8": 8, "psk16": 16, "bpsk": 2, "cross32": 32, "apsk64": 64}
    assert set(want) == set(er.TABLES)
    for name, K in want.items():
        c = er.table(name)
        assert c.size == size[name] and er.grid_k(c) == K, name
    p = er.table("qam16_perm")
    assert not np.array_equal(p, er.qam(16)) and sorted(p.tolist(), key=lambda v: (v.imag, v.real)) \
        == sorted(er.qam(16).tolist(), key=lambda v: (v.imag, v.real))


def test_batch_generator_model():
    """y - H_t x is the noise: its mean square is varn within sampling error, psi_d's direct
    column is ones, the two channel arguments have the norms the docstring states."""
    cons = er.table("cross32")
    b = er.synthetic_batch(cons, 4, 2, 3, 5, 200, 10, seed=2, T_p=14)
    assert np.all(b["psi_d"][:, :, 0] == 1) and np.allclose(np.abs(b["psi_d"]), 1)
    assert np.isclose(b["varn"], np.mean(np.abs(cons) ** 2) / 10.0)
    for i in range(4):
        H = er.heff(b["h"][i], b["psi_d"][i], 2, 3).astype(complex)
        n = b["y_d"][i] - np.einsum("tra,ta->tr", H, b["x_d"][i])
        assert abs(np.mean(np.abs(n) ** 2) / b["varn"] - 1) < 0.2
    assert np.allclose(np.linalg.norm(b["theta_wide"], axis=1), np.linalg.norm(b["h"], axis=1))
    assert np.isclose(np.abs(b["theta_narrow"] - b["h"]).max(), 0.05)
    assert b["theta0"].shape == b["h"].shape and b["u_p"].shape == (4, 14, 12)


@pytest.mark.parametrize("name", ["qam16", "psk16"])
def test_ties_take_the_first_minimum_and_the_uniform_posterior(name):
    cons = er.table(name)
    b = er.synthetic_batch(cons, 1, 3, 4, 2, 3, 10, seed=1)
    z = er.moments(np.zeros_like(b["h"][0]), b["y_d"][0], b["psi_d"][0], cons, 0.3, 3)
    assert np.all(z["gap"] == 0) and np.all(z["mh"] == cons[0])
    mu, e = cons.mean(), np.mean(np.abs(cons) ** 2)
    S = np.full((3, 3), abs(mu) ** 2, dtype=complex) + (e - abs(mu) ** 2) * np.eye(3)
    assert np.abs(z["m"] - mu).max() < 1e-15 and np.abs(z["S"] - S).max() < 1e-14
    th = b["h"][0].reshape(3, 3, 4).copy()
    th[:, 1, :] = 0                                   # stream 1's column of every H_t
    c = er.moments(th.reshape(-1), b["y_d"][0], b["psi_d"][0], cons, 0.3, 3)
    assert np.all(c["gap"] == 0) and np.all(c["mh"][:, 1] == cons[0])
    assert np.abs(c["m"][:, 1] - mu).max() < 1e-15
