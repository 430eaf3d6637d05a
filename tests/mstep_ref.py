"""Extended-precision restatement of the M-step's normal equations (csrc/mstep.hip,
csrc/mstep_large.hip, csrc/mstep_small.hip: R and B^H), a batch generator with general moments
and a host restatement of rbuild_herm_kernel's staging-segment rule.

TEST INFRASTRUCTURE ONLY.  The sums are np.longdouble / np.clongdouble (x87 extended, 64-bit
mantissa, on the x86 hosts the suite runs on), written as GEMMs like
oracle.em_reduced.mstep_build_gemm: the restatement's own rounding is 2^-11 of a float64 ulp.

Per trial, in the C-ABI layout (psi_d (T_d, P), u_p (T_p, L), y_d (T_d, n_rx), y_p (T_p, n_rx),
m (T_d, n_tx), S (T_d, n_tx, n_tx), L = P n_tx, row l = p n_tx + a):
  R[(p,a),(q,b)] = sum_tp u_p[pa] conj(u_p[qb]) + sum_t psi_t[p] conj(psi_t[q]) S_t[a][b]
  rhs[(p,a),r]   = sum_tp u_p[pa] conj(y_p[r])  + sum_t psi_t[p] m_t[a] conj(y_d[t][r])
R_abs / rhs_abs are the same sums over the absolute values of every factor (float64): the
scale of the elementwise bound

  |dev - ref| <= (T_p + T_d + 8) 2^-53 abs_sum                                   (bound())

Each term is two complex multiplications (each 2 sqrt(2) gamma_2 ~ 2.83 u at most, 5.7 u the
pair), a sum of T terms in any order adds at most (T - 1) u and the epilogue's one combination
about 1 u: (T + 5.7) u abs_sum <= (T + 8) u abs_sum, whatever the chunking (MFMA tiles, FMA
chains, the w = psi_p conj(psi_q) the Hermitian build rounds first).
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53

CONS = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j])      # sbce_dims.m only: the M-step reads no table


# ------------------------------------------------------------------ the restatement
def _build(psi, up, yd, yp, m, S, conj):
    """The two sums by GEMMs in the dtype of the arguments; conj: np.conj, or the identity for
    the sums of absolute values."""
    Td, P = psi.shape
    n_tx = m.shape[1]
    L = P * n_tx
    A = (psi.T[:, None, None, :] * np.transpose(S, (1, 2, 0))[None]).reshape(P * n_tx * n_tx, Td)
    R4 = (A @ conj(psi)).reshape(P, n_tx, n_tx, P)                         # [p, a, b, q]
    R = np.transpose(R4, (0, 1, 3, 2)).reshape(L, L) + up.T @ conj(up)
    rhs = up.T @ conj(yp) + (psi.T[:, None, :] * m.T[None]).reshape(L, Td) @ conj(yd)
    return R, rhs


def build_ref(psi_d, u_p, y_d, y_p, m, S):
    """One trial: R (L, L), rhs (L, n_rx) in np.clongdouble and R_abs, rhs_abs in float64."""
    args = [np.asarray(x) for x in (psi_d, u_p, y_d, y_p, m, S)]
    R, rhs = _build(*(x.astype(CLD) for x in args), np.conj)
    R_abs, rhs_abs = _build(*(np.abs(x) for x in args), lambda x: x)
    return R, rhs, R_abs, rhs_abs


def bound(T_p, T_d, abs_sum):
    """The elementwise bar (module docstring)."""
    return (T_p + T_d + 8) * U * abs_sum


def ratio(dev, ref, T_p, T_d, abs_sum):
    """max over the entries of |dev - ref| / bound: <= 1 passes."""
    err = np.abs(np.asarray(dev).astype(CLD) - ref).astype(np.float64)
    return float((err / bound(T_p, T_d, abs_sum)).max())


# ------------------------------------------------------------------ batch generator
def _cn(g, shape):
    return (g.standard_normal(shape) + 1j * g.standard_normal(shape)) / np.sqrt(2.0)


def _phases(g, B, T, P):
    psi = np.exp(1j * g.uniform(0, 2 * np.pi, (B, T, P)))
    psi[..., 0] = 1.0
    return psi


def general_batch(B, n_tx, n_rx, P, T_p, T_d, seed, break_trial=None):
    """A batch with general moments, tied to no constellation: psi_d and the pilot phases of
    unit modulus with uniform phase and a direct-path column of ones; complex normal pilot
    symbols x_p, u_p = psi_p (x) x_p; S_t = A_t A_t^H + 0.1 I with A_t complex standard normal
    (exactly Hermitian, real distinct diagonals, fully complex off-diagonals); m_t, y_d, y_p
    complex normal, independent of S_t.  break_trial = i adds 0.1 CN(0, 1) to u_p[i]: no longer
    a Kronecker product."""
    g = np.random.default_rng(seed)
    psi_d = _phases(g, B, T_d, P)
    psi_p = _phases(g, B, T_p, P)
    x_p = _cn(g, (B, T_p, n_tx))
    u_p = np.einsum("btp,bta->btpa", psi_p, x_p).reshape(B, T_p, P * n_tx)
    A = _cn(g, (B, T_d, n_tx, n_tx))
    S = A @ np.conj(np.swapaxes(A, -1, -2)) + 0.1 * np.eye(n_tx)
    up = np.triu(S, 1)
    S = up + np.conj(np.swapaxes(up, -1, -2)) + np.real(S * np.eye(n_tx))
    m = _cn(g, (B, T_d, n_tx))
    y_d = _cn(g, (B, T_d, n_rx))
    y_p = _cn(g, (B, T_p, n_rx))
    if break_trial is not None:
        u_p[break_trial] += 0.1 * _cn(g, u_p[break_trial].shape)
    return dict(psi_d=psi_d, psi_p=psi_p, x_p=x_p, u_p=u_p, m=m, S=S, y_d=y_d, y_p=y_p,
                cons=CONS, n_tx=n_tx, n_rx=n_rx, P=P, T_p=T_p, T_d=T_d)


def batch_ref(b):
    """build_ref of every trial of a general_batch: a list of (R, rhs, R_abs, rhs_abs)."""
    return [build_ref(b["psi_d"][i], b["u_p"][i], b["y_d"][i], b["y_p"][i], b["m"][i], b["S"][i])
            for i in range(len(b["y_d"]))]


# ------------------------------------------------------------------ rbuild_herm staging rule
LAYOUTS = ("row", "row+p", "two_rows", "prefix")


def pair_of(pi):
    """(p, q), p >= q, of index pi in the p-major order of the lower triangle's pairs."""
    p = (int(np.sqrt(8.0 * pi + 1.0)) - 1) // 2
    while (p + 1) * (p + 2) // 2 <= pi:
        p += 1
    while p * (p + 1) // 2 > pi:
        p -= 1
    return p, pi - p * (p + 1) // 2


def herm_segments(P, pairs_per_block):
    """The index rule at the head of rbuild_herm_kernel restated: every block of
    pairs_per_block consecutive pairs stages the phases of two index segments [lo1, hi1] and
    [lo2, hi2] (the second possibly empty), in one of four layouts:
      "row"       one row p, its q range ends on the diagonal        [qa, qb]
      "row+p"     one row p, q range short of the diagonal           [qa, qb] + [p, p]
      "two_rows"  rows p, p + 1 with disjoint q ranges               [0, qb] + [qa, p + 1]
      "prefix"    anything else                                      [0, pb]
    Returns dict(layouts: the set that occurs, count: the largest staged count,
    blocks: [(layout, lo1, hi1, lo2, hi2, pi0, pi1)])."""
    npairs = P * (P + 1) // 2
    blocks = []
    for pi0 in range(0, npairs, pairs_per_block):
        pi1 = min(pi0 + pairs_per_block, npairs) - 1
        (pa, qa), (pb, qb) = pair_of(pi0), pair_of(pi1)
        lo1, hi1, lo2, hi2, name = 0, pb, pb + 1, pb, "prefix"
        if pa == pb:
            lo1, hi1, name = qa, qb, "row"
            if pb > qb:
                lo2, name = pb, "row+p"
        elif pb == pa + 1 and qa > qb + 1:
            hi1, lo2, name = qb, qa, "two_rows"
        blocks.append((name, lo1, hi1, lo2, hi2, pi0, pi1))
    return dict(layouts={b[0] for b in blocks},
                count=max((b[2] - b[1] + 1) + (b[4] - b[3] + 1) for b in blocks), blocks=blocks)
