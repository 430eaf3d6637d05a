"""NumPy restatement of the noise-variance update and of the EM loop that carries it
(include/sbce.h sbce_noise_var / sbce_em_noise).  TEST INFRASTRUCTURE ONLY.

Per trial, array inputs as oracle.em_reduced: Y_d (T_d, n_rx), Y_p (T_p, n_rx), U_p (T_p, L),
Psi (P, T_d), theta (K,), m (T_d, n_tx), S (T_d, n_tx, n_tx).
"""
import numpy as np

from oracle.em_reduced import aps_from_cons, estep_moments, heff, mstep_build, mstep_solve
from oracle.pm import pm_moments
from oracle.detectors import detector_moments

STATUS_NOISE = 64


def noise_var_ref(Y_d, Y_p, U_p, Psi, theta, m, S, parts=False):
    """sigma^2 = Q / (n_rx (T_p + T_d)) with
    Q = sum_p ||y_p - H_c u_p||^2 + sum_t ( ||y_t - H_t m_t||^2 + tr(H_t C_t H_t^H) ),
    C_t = S_t - m_t m_t^H, H_t[r, a] = sum_p Psi[p, t] theta[(p n_tx + a) n_rx + r].
    parts=True: (sigma^2, Q, sum ||y||^2)."""
    T_d, n_rx = Y_d.shape
    T_p = Y_p.shape[0]
    n_tx = m.shape[1]
    theta = np.asarray(theta, dtype=complex).reshape(-1)
    H = heff(theta, Psi, n_tx, n_rx)                          # (T_d, n_rx, n_tx)
    e = Y_d - np.einsum("tra,ta->tr", H, m)
    C = S - m[:, :, None] * np.conj(m)[:, None, :]
    tr = np.einsum("tra,tab,trb->", H, C, np.conj(H)).real
    Q = float(np.sum(np.abs(e) ** 2) + tr)
    if T_p:
        ep = Y_p - U_p @ theta.reshape(-1, n_rx)                 # (H_c u_p)[r] = sum_l theta[l n_rx + r] u[l]
        Q += float(np.sum(np.abs(ep) ** 2))
    s2 = Q / (n_rx * (T_p + T_d))
    if parts:
        return s2, Q, float(np.sum(np.abs(Y_d) ** 2) + np.sum(np.abs(Y_p) ** 2))
    return s2


def moments(theta, Y_d, Psi, cons, varn, n_tx, mode, partition_r=0):
    """The E-step of `mode` with the parameter varn (the posterior divides by varn^2)."""
    n_rx = Y_d.shape[1]
    if mode in ("soft", "hard"):
        return estep_moments(theta, Y_d, Psi, aps_from_cons(cons, n_tx), varn, mode)[:2]
    if mode in ("pm", "pm_soft"):
        return pm_moments(theta, Y_d, Psi, cons, n_tx, n_rx, partition_r, varn, mode == "pm_soft")
    if mode in ("zf", "mmse"):
        return detector_moments(theta, Y_d, Psi, aps_from_cons(cons, n_tx), varn, n_tx, n_rx, mode)
    raise ValueError(mode)


def apply_rules(Q, denom, prev, varn_min):
    """(new parameter, status flag) of one update: the floor and the keep-previous rule."""
    if not np.isfinite(Q):
        return prev, STATUS_NOISE
    s2 = Q / denom
    if s2 < varn_min * varn_min:
        return varn_min, STATUS_NOISE
    return float(np.sqrt(s2)), 0


def em_noise_ref(Y_d, Y_p, U_p, Psi, cons, varn, itera, theta0, n_tx, mode="soft", partition_r=0,
                 varn_min=1e-6, h=None):
    """sbce_em_noise over one trial: per iteration E-step (parameter v), M-step (np.linalg.solve),
    noise update, then the oracle early stop |‖theta‖ - ‖h‖| < 1 after an iteration l != 0.
    Returns dict(theta, varn, hist (itera,), iters_done, status, trace [(theta, v) after each
    iteration])."""
    T_d, n_rx = Y_d.shape
    denom = n_rx * (Y_p.shape[0] + T_d)
    theta = np.asarray(theta0, dtype=complex).reshape(-1)
    v = float(varn)
    hist = np.zeros(itera)
    status, done, trace = 0, 0, []
    for l in range(itera):
        m, S = moments(theta, Y_d, Psi, cons, v, n_tx, mode, partition_r)
        R, rhs = mstep_build(U_p, Y_p, Psi, Y_d, m, S)
        theta = mstep_solve(R, rhs)
        _, Q, _ = noise_var_ref(Y_d, Y_p, U_p, Psi, theta, m, S, parts=True)
        v, flag = apply_rules(Q, denom, v, varn_min)
        status |= flag
        hist[l:] = v                       # a stopped trial's later entries stay at its last value
        trace.append((theta.copy(), v))
        done = l + 1
        if h is not None and abs(np.linalg.norm(theta) - np.linalg.norm(h)) < 1 and l != 0:
            break
    return dict(theta=theta, varn=v, hist=hist, iters_done=done, status=status, trace=trace)


def loglik_soft(Y_d, Y_p, U_p, Psi, cons, theta, v, n_tx):
    """Observed-data log-likelihood of (theta, sigma^2 = v^2) under uniform symbols: the pilots'
    Gaussian terms plus, per data symbol, log (1/J) sum_j CN(y_t; H_t x_j, sigma^2 I)."""
    T_d, n_rx = Y_d.shape
    s2 = v * v
    theta = np.asarray(theta, dtype=complex).reshape(-1)
    aps = aps_from_cons(cons, n_tx)
    H = heff(theta, Psi, n_tx, n_rx)
    d = np.sum(np.abs(Y_d[:, None, :] - np.einsum("tra,ja->tjr", H, aps)) ** 2, axis=2)   # (T_d, J)
    dm = d.min(axis=1)
    ll = np.sum(-dm / s2 + np.log(np.sum(np.exp(-(d - dm[:, None]) / s2), axis=1)))
    ll -= T_d * (np.log(aps.shape[0]) + n_rx * np.log(np.pi * s2))
    ep = Y_p - U_p @ theta.reshape(-1, n_rx)
    ll += -np.sum(np.abs(ep) ** 2) / s2 - Y_p.shape[0] * n_rx * np.log(np.pi * s2)
    return float(ll)
