"""NumPy restatement of the semi-blind Gaussian-approximation EM, the comparator EM_approx of
"Comparision/Comparision T_d vs NMSE.py":106-145 (the same function at "Comparision/
Comparision T_p .py":74-113), in the form the device kernel computes (csrc/approx.hip).

Test infrastructure only: the product package never imports it.  Reference layouts:
PsiTilde_tp N x L_p, PsiTilde_td N x L_d, x_p (L_p, 1), Y_p M x L_p, Y_d M x L_d, G N x M.
"""
import numpy as np


def initial_g(Psi_p, x_p, Y_p):
    """G_0 = conj(Y_p pinv(Psi_p diag(x_p)))^T (:107-108)."""
    S_p = np.matmul(Psi_p, np.diagflat(x_p))
    return np.conjugate(np.matmul(Y_p, np.linalg.pinv(S_p))).T


def pilot_terms(Psi_p, x_p, Y_p):
    """A_p = sum_p |x_p|^2 psi_p psi_p^H (:119-120), Rows_p = sum_p Y_p[:, p] conj(x_p) psi_p^H
    (:136-137): constant over the iterations."""
    x = np.asarray(x_p).reshape(-1)
    A_p = (Psi_p * np.abs(x) ** 2) @ Psi_p.conj().T
    Rows_p = (Y_p * x.conj()) @ Psi_p.conj().T
    return A_p, Rows_p


def update(G, Psi_d, Y_d, A_p, Rows_p, varn):
    """One update from G (steps 1-7).  Returns (G_new, A, Rows, mu)."""
    v2 = varn ** 2
    g = G.conj().T @ Psi_d                               # M x L_d: g_t = G^H psi_t
    a = np.sum(np.abs(g) ** 2, axis=0)
    mu = np.sum(g.conj() * Y_d, axis=0) / (a + v2)       # g_t^H y_t / (a_t + v^2)  (:122-126)
    q = np.sum((G.T @ Psi_d) * g, axis=0)                # plain transpose (:128): complex
    c = v2 / (q + v2) + np.abs(mu) ** 2                  # (:129-131)
    A = A_p + (Psi_d * c) @ Psi_d.conj().T               # (:132): not Hermitian
    Rows = Rows_p + (Y_d * mu.conj()) @ Psi_d.conj().T   # (:138-139)
    G_new = np.linalg.solve(A.T, Rows.T).conj()          # (Rows A^-1)^H  (:140-141)
    return G_new, A, Rows, mu


def em_approx(Psi_p, Psi_d, x_p, Y_p, Y_d, updates, varn, G0=None, first=False):
    """`updates` updates from G_0 (the reference performs Iterations + 1, `while i <=
    Iterations`).  first=True also returns (A, Rows, mu) of the first update."""
    G = initial_g(Psi_p, x_p, Y_p) if G0 is None else np.asarray(G0, dtype=complex)
    A_p, Rows_p = pilot_terms(Psi_p, x_p, Y_p)
    keep = None
    for i in range(updates):
        G, A, Rows, mu = update(G, Psi_d, Y_d, A_p, Rows_p, varn)
        if i == 0:
            keep = (A, Rows, mu)
    return (G,) + keep if first else G


def batch_major(Psi_p, Psi_d, x_p, Y_p, Y_d, G0):
    """One trial's reference-layout arrays as the (1, ...) batch-major arrays of
    sbce_approx_em / em_approx_batch."""
    return dict(y_d=Y_d.T[None], y_p=Y_p.T[None], psi_d=Psi_d.T[None], psi_p=Psi_p.T[None],
                x_p=np.asarray(x_p).reshape(1, -1), g0=np.asarray(G0)[None])
