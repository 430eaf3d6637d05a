"""CPU tier of the soft ZF / MMSE EM chain: guards on the seeded batches of
tests/linear_em_oracle.py, which the GPU tier (tests/test_gpu_estep_linear.py) compares the device
chain against at 1e-9, and the restated chain's own gain over the pilot-only start."""
import numpy as np
import pytest

import linear_em_oracle as eo

PERTURB = 1e-13


def _perturbed(c, b):
    rs = np.random.RandomState(1000 + b)
    th = c["theta0"][b]
    return th * (1 + PERTURB * np.exp(2j * np.pi * rs.rand(th.size)))


@pytest.mark.parametrize("shape,vi,kind", eo.CHAINS, ids=eo.chain_id)
def test_chain_is_well_conditioned(shape, vi, kind):
    """What keeps a 1e-9 comparison of 4 iterations meaningful: no symbol of any iteration has a
    failed pivot, every cond(A) <= 2e3, and a relative 1e-13 perturbation of theta0 stays within
    1e3 x 1e-13 after each iteration (seen at most x 78: MMSE at (6, 8, 13, 90); cond(A) at most
    1985, at (5, 6, 3, 20))."""
    c = eo.batch(shape, vi)
    worst_amp = worst_kappa = 0.0
    for b, r in enumerate(eo.chain_ref(shape, vi, kind)):
        assert not r["fail"]
        p = eo.chain(c, b, kind, eo.ITERS, theta0=_perturbed(c, b))
        assert not p["fail"]
        amp = max(np.linalg.norm(x - y) / np.linalg.norm(x)
                  for x, y in zip(r["thetas"], p["thetas"])) / PERTURB
        worst_amp, worst_kappa = max(worst_amp, amp), max(worst_kappa, r["kappa"], p["kappa"])
    print(f"{shape} varn {eo.VARNS[vi]} {kind}: perturbation x {worst_amp:.3g}, "
          f"max cond(A) {worst_kappa:.4g}")
    assert worst_kappa <= 2e3
    assert worst_amp <= 1e3


@pytest.mark.parametrize("shape,kind", [(eo.S56, "mmse"), (eo.S56, "zf"), (eo.S34, "mmse"),
                                        (eo.S34, "zf")], ids=eo.chain_id)
def test_chain_improves_on_the_pilot_only_start(shape, kind):
    """varn = 0.3: four iterations at least halve the NMSE of the pilot least-squares start on
    every trial (the smallest gain on these seeds is x 6.4: (5, 6, 3, 20))."""
    c = eo.batch(shape, 0)
    for b, r in enumerate(eo.chain_ref(shape, 0, kind)):
        start, final = eo.nmse_of(c, b, c["theta0"][b]), eo.nmse_of(c, b, r["thetas"][-1])
        print(f"{shape} {kind} trial {b}: NMSE {start:.3e} -> {final:.3e} (x {start / final:.2f})")
        assert final < 0.5 * start


def test_batches_are_the_model():
    """The generator's own contract: Kronecker pilots, unit-modulus phases, theta0 solves the
    pilot least-squares problem."""
    for shape in eo.SHAPES:
        c = eo.batch(shape, 0)
        n_tx, n_rx, P, T_p, M = shape
        assert c["y_d"].shape == (eo.B, eo.T_D, n_rx) and c["u_p"].shape == (eo.B, T_p, P * n_tx)
        assert np.allclose(np.abs(c["psi_d"]), 1.0, rtol=0, atol=1e-15)
        u = c["u_p"].reshape(eo.B, T_p, P, n_tx)
        assert np.allclose(u[:, :, 1:] * u[:, :, :1, :1], u[:, :, :1] * u[:, :, 1:, :1], rtol=0, atol=1e-12)
        for b in range(eo.B):
            g = c["u_p"][b].conj().T @ (c["u_p"][b] @ c["theta0"][b].reshape(-1, n_rx) - c["y_p"][b])
            assert np.abs(g).max() <= 1e-9 * np.abs(c["u_p"][b].conj().T @ c["y_p"][b]).max()
