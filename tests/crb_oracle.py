"""NumPy oracle of the Cramer-Rao bounds (sbce_crb, include/sbce.h).

Reduced form: y = H_c u + n with u = psi (x) x (index l = p n_tx + a) and n ~ CN(0, sigma2 I).
With the regressors known, each row of the least-squares estimate of H_c has covariance
sigma2 R^-1, R = sum_p u_p u_p^H + sum_t (psi_t psi_t^H) (x) S_t, so

    E||theta_hat - theta||^2 = n_rx sigma2 tr(R^-1),      var(theta_hat[l n_rx + r]) = sigma2 (R^-1)_ll.

``fisher_full`` is the independent check: the K x K Fisher matrix of theta = vec(H_c)
(theta[l n_rx + r] = H_c[r, l]) from the n_rx x K regressor matrices Z = u^T (x) I_{n_rx} -- the
Kronecker form the reference writes its model in, y = Z theta + n -- inverted as a whole.
"""
import numpy as np

PIVOT_REL = 1e-14      # the project's pivot rule: a pivot must exceed PIVOT_REL * max diag R


def genie_S(x_d):
    """S_t = x_t x_t^H of known symbols x_d (..., n_tx)."""
    x = np.asarray(x_d, dtype=complex)
    return x[..., :, None] * np.conj(x[..., None, :])


def normal_matrix(u_p, psi_d, S):
    """R (L, L) of one trial: u_p (T_p, L), psi_d (T_d, P), S (T_d, n_tx, n_tx)."""
    u_p, psi_d, S = (np.asarray(a, dtype=complex) for a in (u_p, psi_d, S))
    P, n_tx = psi_d.shape[1], S.shape[1]
    L = P * n_tx
    R = np.einsum("tl,tk->lk", u_p, np.conj(u_p)) if u_p.shape[0] else np.zeros((L, L), complex)
    # ((p, a), (q, c)) = sum_t psi_tp conj(psi_tq) S_t[a, c]
    T = psi_d.shape[0]
    pq = (psi_d[:, :, None] * np.conj(psi_d)[:, None, :]).reshape(T, P * P)
    D = (pq.T @ S.reshape(T, n_tx * n_tx)).reshape(P, P, n_tx, n_tx)
    return R + np.transpose(D, (0, 2, 1, 3)).reshape(L, L)


def chol_pivots(R):
    """The pivots d_c = R_cc - sum_{k<c} |G_ck|^2 of an unblocked lower Cholesky, replayed until the
    first one that fails the rule (later entries are NaN): (pivots, identifiable)."""
    A = np.array(R, dtype=complex)
    L = A.shape[0]
    tol = PIVOT_REL * np.max(np.real(np.diag(A)))
    piv = np.full(L, np.nan)
    for c in range(L):
        d = A[c, c].real
        piv[c] = d
        if not d > tol:
            return piv, False
        g = np.sqrt(d)
        A[c + 1:, c] /= g
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], np.conj(A[c + 1:, c]))
    return piv, True


def crb_reduced(u_p, psi_d, S, n_rx, sigma2):
    """dict(R, identifiable, diag_inv (L,), tr_inv, mse, cond) of one trial by the reduced form and
    the pivot rule: an unidentifiable trial has every value +inf."""
    R = normal_matrix(u_p, psi_d, S)
    L = R.shape[0]
    _, ok = chol_pivots(R)
    if not ok:
        inf = np.inf
        return dict(R=R, identifiable=False, diag_inv=np.full(L, inf), tr_inv=inf, mse=inf, cond=inf)
    d = np.real(np.diag(np.linalg.inv(R)))
    tr = float(np.sum(d))
    return dict(R=R, identifiable=True, diag_inv=d, tr_inv=tr, mse=n_rx * sigma2 * tr,
                cond=float(np.linalg.cond(R)))


def regressor_matrix(u, n_rx):
    """Z (n_rx, K) with y = Z theta for theta[l n_rx + r] = H_c[r, l]: u^T (x) I_{n_rx}."""
    return np.kron(np.asarray(u, dtype=complex)[None, :], np.eye(n_rx))


def fisher_full(u_p, psi_d, x_d, n_rx, sigma2):
    """K x K Fisher matrix of theta with every regressor known (pilots u_p (T_p, L), data
    u_t = psi_t (x) x_t from psi_d (T_d, P) and x_d (T_d, n_tx)): J = sum Z^H Z / sigma2."""
    us = [np.asarray(u, dtype=complex) for u in u_p]
    us += [np.kron(p, x) for p, x in zip(np.asarray(psi_d, complex), np.asarray(x_d, complex))]
    K = us[0].size * n_rx
    J = np.zeros((K, K), dtype=complex)
    for u in us:
        Z = regressor_matrix(u, n_rx)
        J += np.conj(Z.T) @ Z
    return J / sigma2


def crb_fisher(u_p, psi_d, x_d, n_rx, sigma2):
    """(E||theta_hat - theta||^2, per-coefficient variances (K,)) from the inverse of fisher_full."""
    C = np.linalg.inv(fisher_full(u_p, psi_d, x_d, n_rx, sigma2))
    v = np.real(np.diag(C))
    return float(np.sum(v)), v


def ls_known(y, U, n_rx):
    """Least-squares theta (K,) from y (T, n_rx) and known regressors U (T, L): Y = U H_c^T, so lstsq
    gives H_c^T (L, n_rx), whose row-major flattening is theta[l n_rx + r] = H_c[r, l]."""
    Hc = np.linalg.lstsq(np.asarray(U, complex), np.asarray(y, complex), rcond=None)[0]   # (L, n_rx)
    return Hc.reshape(-1)
