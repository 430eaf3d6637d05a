"""NumPy restatement of the EM chain on the soft ZF / MMSE E-steps (include/sbce.h
SBCE_ESTEP_MMSE_SOFT / SBCE_ESTEP_ZF_SOFT), one trial at a time: the E-step's moments are
linear_oracle.linear_ref's (sigma2 = varn^2, es = mean |cons|^2), the M-step is
oracle.em_reduced's mstep_build + mstep_solve, the noise variant adds noise_oracle's update.  Also
the seeded batches the CPU and GPU tests share.  Test infrastructure only: the product has no CPU
path."""
import functools

import numpy as np

import linear_oracle as lo
import noise_oracle as no
from oracle.em_reduced import mstep_build, mstep_solve, nmse

B = 3
T_D = 40                  # one full 32-symbol workgroup and a ragged one of 8 per trial
ITERS = 4
VARNS = (0.3, 1.0)
# (n_tx, n_rx, P, T_p, M): each takes another M-step route
#   (3, 4, 2, 8)    L = 6: the two-launch small path
#   (5, 6, 3, 20)   L = 15: the single-launch small M-step
#   (8, 8, 5, 48)   n_tx = 8: MFMA build and batched Cholesky, the fixed-point freeze armed
#   (6, 8, 13, 90)  L = 78 > 64: past the small M-step
SHAPES = ((3, 4, 2, 8, 16), (5, 6, 3, 20, 16), (8, 8, 5, 48, 4), (6, 8, 13, 90, 16))
S34, S56, S88, S68 = SHAPES
# one seed per shape, chosen (tests/test_linear_em.py asserts it) so that in every iteration of
# every chain below no symbol has a failed pivot, every cond(A) <= 2e3 and a relative 1e-13
# perturbation of theta0 grows by at most 1e3
SEEDS = {S34: 1, S56: 1, S88: 1, S68: 1}
# ZF only where n_rx > n_tx: at 8 x 8 its cond(A) reaches 1e4..1e5 and the chain multiplies a
# perturbation by > 100 in 4 iterations -- nothing a 1e-9 comparison could pin
CHAINS = tuple((s, vi, kind) for s in SHAPES for vi in range(len(VARNS))
               for kind in (("mmse", "zf") if s[1] > s[0] else ("mmse",)))


def chain_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def batch(shape, vi, seed=None):
    """B trials drawn from the model at noise variance varn^2: theta ~ CN(0, 1/P), unit-modulus
    random phases for data and pilots, uniform table symbols, Kronecker pilots u_p = psi_p (x) x_p,
    theta0 = the pilot least-squares solution."""
    n_tx, n_rx, P, T_p, M = shape
    varn = VARNS[vi]
    rs = np.random.RandomState(SEEDS[shape] if seed is None else seed)
    cons, _ = lo.table(M)
    K = P * n_tx * n_rx
    h = (rs.randn(B, K) + 1j * rs.randn(B, K)) / np.sqrt(2 * P)
    psi_d = np.exp(2j * np.pi * rs.rand(B, T_D, P))
    psi_p = np.exp(2j * np.pi * rs.rand(B, T_p, P))
    x_d = cons[rs.randint(0, M, size=(B, T_D, n_tx))]
    x_p = cons[rs.randint(0, M, size=(B, T_p, n_tx))]
    u_p = (psi_p[:, :, :, None] * x_p[:, :, None, :]).reshape(B, T_p, P * n_tx)
    H = np.einsum("btp,bpar->btra", psi_d, h.reshape(B, P, n_tx, n_rx))
    sd = np.sqrt(varn * varn / 2)
    y_d = np.einsum("btra,bta->btr", H, x_d) + sd * (rs.randn(B, T_D, n_rx) + 1j * rs.randn(B, T_D, n_rx))
    y_p = np.einsum("btl,blr->btr", u_p, h.reshape(B, P * n_tx, n_rx)) \
        + sd * (rs.randn(B, T_p, n_rx) + 1j * rs.randn(B, T_p, n_rx))
    theta0 = np.stack([np.linalg.lstsq(u_p[b], y_p[b], rcond=None)[0].reshape(-1) for b in range(B)])
    c = dict(y_d=y_d, y_p=y_p, psi_d=psi_d, u_p=u_p, cons=cons, theta0=theta0, h=h, x_d=x_d,
             n_tx=n_tx, n_rx=n_rx, varn=varn)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def estep(c, b, theta, kind, varn):
    """(m (T_d, n_tx), S (T_d, n_tx, n_tx), linear_ref's dict) of trial b at theta."""
    n_tx = c["n_tx"]
    o = lo.linear_ref(c["y_d"][b:b + 1], c["psi_d"][b:b + 1], c["cons"], theta[None], varn * varn,
                      n_tx, kind=kind, es=None)
    mom = o["moments"][0]
    return mom[:, :n_tx], mom[:, n_tx:].reshape(-1, n_tx, n_tx), o


def mstep(c, b, m, S):
    return mstep_solve(*mstep_build(c["u_p"][b], c["y_p"][b], c["psi_d"][b].T, c["y_d"][b], m, S))


def chain(c, b, kind, iters, theta0=None, varn=None):
    """The restated sbce_em of trial b: dict(thetas [theta after each iteration], kappa = the
    largest cond(A) met, fail = a symbol had a failed pivot)."""
    theta = np.array(c["theta0"][b] if theta0 is None else theta0, dtype=complex)
    varn = c["varn"] if varn is None else varn
    thetas, kappa, fail = [], 0.0, False
    for _ in range(iters):
        m, S, o = estep(c, b, theta, kind, varn)
        kappa, fail = max(kappa, float(o["kappa"].max())), fail or bool(o["fail"].any())
        theta = mstep(c, b, m, S)
        thetas.append(theta)
    return dict(thetas=thetas, kappa=kappa, fail=fail)


@functools.lru_cache(maxsize=None)
def chain_ref(shape, vi, kind, iters=ITERS):
    """chain() of every trial of batch(shape, vi), computed once and shared (never modified)."""
    c = batch(shape, vi)
    return tuple(chain(c, b, kind, iters) for b in range(B))


@functools.lru_cache(maxsize=None)
def noise_chain_ref(shape, vi, kind, iters, start, varn_min=1e-6):
    """The restated sbce_em_noise (noise_oracle.em_noise_ref's loop on this E-step) of every
    trial: tuple of dict(theta, varn, hist (iters,), status)."""
    c = batch(shape, vi)
    out = []
    for b in range(B):
        denom = c["n_rx"] * (c["y_p"].shape[1] + T_D)
        theta, v, status = np.array(c["theta0"][b]), float(start), 0
        hist = np.zeros(iters)
        for l in range(iters):
            m, S, _ = estep(c, b, theta, kind, v)
            theta = mstep(c, b, m, S)
            _, Q, _ = no.noise_var_ref(c["y_d"][b], c["y_p"][b], c["u_p"][b], c["psi_d"][b].T, theta,
                                       m, S, parts=True)
            v, flag = no.apply_rules(Q, denom, v, varn_min)
            status |= flag
            hist[l:] = v
        out.append(dict(theta=theta, varn=v, hist=hist, status=status))
    return tuple(out)


def nmse_of(c, b, theta):
    return nmse(theta, c["h"][b])
