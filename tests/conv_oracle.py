"""NumPy restatement of the observed-data log-likelihood and of the EM loop with the truth-free
convergence stop (include/sbce.h sbce_loglik / sbce_em_conv).  TEST INFRASTRUCTURE ONLY.

Per trial, array inputs as noise_oracle: Y_d (T_d, n_rx), Y_p (T_p, n_rx), U_p (T_p, L),
Psi (P, T_d), theta (K,).
"""
import numpy as np

from oracle.em_reduced import aps_from_cons, heff, mstep_build, mstep_solve
import noise_oracle as nz

STATUS_CONVERGED = 128


def _dist(Y_d, Psi, cons, theta, n_tx):
    """d[t, j] = ||y_t - H_t x_j||^2 over the hypotheses in product order, and max_j ||H_t x_j||."""
    n_rx = Y_d.shape[1]
    aps = aps_from_cons(cons, n_tx)
    H = heff(np.asarray(theta, dtype=complex).reshape(-1), Psi, n_tx, n_rx)
    Hx = np.einsum("tra,ja->tjr", H, aps)
    d = np.sum(np.abs(Y_d[:, None, :] - Hx) ** 2, axis=2)
    return d, np.sqrt(np.sum(np.abs(Hx) ** 2, axis=2)).max(axis=1)


def loglik_sym_ref(Y_d, Psi, cons, theta, v, n_tx):
    """ll_sym[t] = -d_min/s2 + log sum_j e^{-(d_j - d_min)/s2} - log J - n_rx log(pi s2)."""
    s2 = v * v
    d, _ = _dist(Y_d, Psi, cons, theta, n_tx)
    dm = d.min(axis=1)
    return (-dm / s2 + np.log(np.sum(np.exp(-(d - dm[:, None]) / s2), axis=1)) - np.log(d.shape[1])
            - Y_d.shape[1] * np.log(np.pi * s2))


def loglik_ref(Y_d, Y_p, U_p, Psi, cons, theta, v, n_tx):
    """The trial's log-likelihood: noise_oracle.loglik_soft."""
    return nz.loglik_soft(Y_d, Y_p, U_p, Psi, cons, theta, v, n_tx)


def error_scale(Y_d, Y_p, U_p, Psi, cons, theta, v, n_tx):
    """(A, A_t (T_d,)): the magnitudes a rounding error of the log-likelihood scales with,
    A = sum_t (||y_t|| + max_j ||H_t x_j||)^2 / s2 + sum_p (||y_p|| + ||H_c u_p||)^2 / s2
        + (T_d + T_p) n_rx |log(pi s2)| + T_d log J,          A_t = the data symbol t's share."""
    T_d, n_rx = Y_d.shape
    T_p = Y_p.shape[0]
    s2 = v * v
    d, hx = _dist(Y_d, Psi, cons, theta, n_tx)
    lc = n_rx * abs(np.log(np.pi * s2))
    A_t = (np.linalg.norm(Y_d, axis=1) + hx) ** 2 / s2 + lc + np.log(d.shape[1])
    A = A_t.sum()
    if T_p:
        hu = U_p @ np.asarray(theta, dtype=complex).reshape(-1, n_rx)
        A += np.sum((np.linalg.norm(Y_p, axis=1) + np.linalg.norm(hu, axis=1)) ** 2) / s2 + T_p * lc
    return float(A), A_t


def em_conv_ref(Y_d, Y_p, U_p, Psi, cons, varn, itera, theta0, n_tx, mode="soft", partition_r=0,
                tol_theta=1e-6, tol_ll=0.0, min_iters=2, estimate_noise=False, varn_min=1e-6,
                loglik=False):
    """sbce_em_conv over one trial: per iteration E-step (parameter v), M-step (np.linalg.solve),
    the noise update (estimate_noise), the log-likelihood at the new theta and the current v
    (loglik), then the decision: stop when l + 1 >= min_iters and
      ||theta_l - theta_{l-1}||^2 <= tol_theta^2 ||theta_l||^2          (theta_{-1} = theta0), or
      tol_ll > 0, l >= 1 and ll_l - ll_{l-1} <= tol_ll |ll_l|.
    Returns dict(theta, varn, iters_done, status, dtheta_hist, ll_hist, hist, delta, dll): the
    histories (itera,) with a stopped trial's later entries at their last value; delta / dll the
    ratios sqrt(||dtheta||^2 / ||theta||^2) / tol_theta and (ll_l - ll_{l-1}) / (tol_ll |ll_l|) of
    every iteration performed (how far each decision was from its threshold); trace [(theta, v)
    after each iteration performed]."""
    T_d, n_rx = Y_d.shape
    denom = n_rx * (Y_p.shape[0] + T_d)
    theta = np.asarray(theta0, dtype=complex).reshape(-1)
    v = float(varn)
    dth, llh, hist = np.zeros(itera), np.zeros(itera), np.zeros(itera)
    status, done, delta, dll, trace = 0, 0, [], [], []
    for l in range(itera):
        prev = theta
        m, S = nz.moments(theta, Y_d, Psi, cons, v, n_tx, mode, partition_r)
        R, rhs = mstep_build(U_p, Y_p, Psi, Y_d, m, S)
        theta = mstep_solve(R, rhs)
        if estimate_noise:
            _, Q, _ = nz.noise_var_ref(Y_d, Y_p, U_p, Psi, theta, m, S, parts=True)
            v, flag = nz.apply_rules(Q, denom, v, varn_min)
            status |= flag
        hist[l:] = v
        nd, nt = np.sum(np.abs(theta - prev) ** 2), np.sum(np.abs(theta) ** 2)
        dth[l:] = np.sqrt(nd / nt)
        stop = nd <= tol_theta * tol_theta * nt
        if tol_theta > 0:
            delta.append(float(dth[l] / tol_theta))
        if loglik:
            ll = loglik_ref(Y_d, Y_p, U_p, Psi, cons, theta, v, n_tx)
            if tol_ll > 0 and l >= 1:
                dll.append(float((ll - llh[l - 1]) / (tol_ll * abs(ll))))
                stop = stop or ll - llh[l - 1] <= tol_ll * abs(ll)
            llh[l:] = ll
        trace.append((theta.copy(), v))
        done = l + 1
        if stop and done >= min_iters:
            status |= STATUS_CONVERGED
            break
    return dict(theta=theta, varn=v, iters_done=done, status=status, dtheta_hist=dth,
                ll_hist=llh if loglik else None, hist=hist, delta=delta, dll=dll, trace=trace)
