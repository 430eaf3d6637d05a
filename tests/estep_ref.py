"""Extended-precision restatement of the exact E-step's posterior moments (include/sbce.h,
SBCE_ESTEP_SOFT / SBCE_ESTEP_HARD) for ANY constellation table, the tables the E-step tests run
and a batch generator that takes a table (signal_model.synthetic_batch is square-QAM only).

TEST INFRASTRUCTURE ONLY.  Everything is np.longdouble / np.clongdouble (x87 extended, 64-bit
mantissa, on the x86 hosts the suite runs on): the restatement's own rounding is ~1e-19 per
operation, five orders below the 1e-11 max|c|^2 the device is held to.

Per data symbol t, with H_t[r][a] = sum_p psi_d[t][p] theta[(p n_tx + a) n_rx + r]:
  d_j = ||y_t - H_t x_j||^2 over the J = M^n_tx hypotheses in itertools.product order (first
        stream slowest),
  soft: w_j = exp(-(d_j - d_min) / varn^2) (the posterior denominator is varn SQUARED),
        m_t = sum w x / sum w,  S_t[a][b] = sum w x_a conj(x_b) / sum w,
  hard: j^ = np.argmin(d) (first minimum), m_t = x_j^, S_t = x_j^ x_j^^H,
  gap  = (d_second - d_min) / d_min, d_second the second smallest entry of d (0 on a tie).
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble


# ------------------------------------------------------------------ tables
def qam(M):
    """Square M-QAM in the package's table order (qam.qam_constellation: in-phase fastest)."""
    L = int(round(np.sqrt(M)))
    assert L * L == M
    lv = np.arange(-L + 1, L, 2).astype(float)
    return (lv[None, :] + 1j * lv[:, None]).reshape(-1)


def psk(M):
    return np.exp(2j * np.pi * np.arange(M) / M)


def _qam16_perm():
    return qam(16)[np.random.default_rng(1234).permutation(16)]


def _qam64_perm():
    # this draw puts 1 + 1j first of the four innermost points: at z = 0 the first minimum in table
    # order is then not the point lowest on both axes, which a per-axis search meets first
    return qam(64)[np.random.default_rng(4324).permutation(64)]


def _qam16_uneven():
    re = np.array([-3.0, -1.0, 1.5, 4.0])
    im = np.array([-2.5, -1.0, 0.5, 3.0])
    return (re[None, :] + 1j * im[:, None]).reshape(-1)


def _cross32():
    lv = np.arange(-5, 6, 2).astype(float)
    g = (lv[None, :] + 1j * lv[:, None]).reshape(-1)
    return g[~((np.abs(g.real) == 5) & (np.abs(g.imag) == 5))]


def _apsk64():
    rings = [np.float64(r) * np.exp(2j * np.pi * (np.arange(16) + 0.25 * k) / 16)
             for k, r in enumerate((1.0, 2.0, 3.0, 4.0))]
    return np.concatenate(rings)


TABLES = {
    "qam16": lambda: qam(16),
    "qam64": lambda: qam(64),
    "qam16_perm": _qam16_perm,                       # a grid (K = 4), permuted table order
    "qam64_perm": _qam64_perm,                       # a grid (K = 8), permuted table order
    "qam16_uneven": _qam16_uneven,                   # a grid (K = 4), unequal spacing, off centre
    "qam16_rot": lambda: qam(16) * np.exp(0.3j),     # no grid (K = 0)
    "psk8": lambda: psk(8),
    "psk16": lambda: psk(16),
    "bpsk": lambda: np.array([1.0 + 0j, -1.0 + 0j]),
    "cross32": _cross32,                             # the 6 x 6 grid minus its corners
    "apsk64": _apsk64,                               # four rings of 16 points
}


def table(name):
    c = np.ascontiguousarray(TABLES[name](), dtype=np.complex128)
    assert len(set(c.tolist())) == c.size
    return c


def grid_k(cons):
    """csrc/sbce_internal.h grid_build restated: K > 0 when the table is a K x K grid of real and
    imaginary levels in any order (K <= 8), else 0 (the exhaustive fallbacks run)."""
    cons = np.asarray(cons)
    M = cons.size
    K = int(round(np.sqrt(M)))
    if K * K != M or K > 8:
        return 0
    for v in cons:
        lt_x, eq_x = np.sum(cons.real < v.real), np.sum(cons.real == v.real)
        lt_y, eq_y = np.sum(cons.imag < v.imag), np.sum(cons.imag == v.imag)
        if not (eq_x == K and eq_y == K and np.sum(cons == v) == 1 and lt_x % K == 0
                and lt_y % K == 0):
            return 0
    return K


# ------------------------------------------------------------------ the restatement
def heff(theta, psi_d, n_tx, n_rx):
    """(T, n_rx, n_tx) effective channels in extended precision; psi_d is (T, P)."""
    psi = np.asarray(psi_d).astype(CLD)
    H3 = np.asarray(theta).astype(CLD).reshape(psi.shape[1], n_tx, n_rx)       # [p, a, r]
    H = np.zeros((psi.shape[0], n_rx, n_tx), dtype=CLD)
    for p in range(psi.shape[1]):
        H += psi[:, p, None, None] * H3[p].T[None]
    return H


def _hyp(cons, n_tx, j0, j1):
    """Hypotheses j0..j1-1 of the product table: (j1 - j0, n_tx) table indices."""
    M = cons.size
    j = np.arange(j0, j1, dtype=np.int64)
    return np.stack([(j // M ** (n_tx - 1 - a)) % M for a in range(n_tx)], axis=1)


def symbol_moments(H, y, cons, varn, chunk=1 << 16):
    """One symbol: dict(m, S (soft), mh, Sh, jh (hard), gap).  H (n_rx, n_tx), y (n_rx,) extended."""
    n_rx, n_tx = H.shape
    c = np.asarray(cons).astype(CLD)
    J = cons.size ** n_tx
    d = np.empty(J, dtype=LD)
    for j0 in range(0, J, chunk):
        x = c[_hyp(cons, n_tx, j0, min(J, j0 + chunk))]
        r = np.broadcast_to(y[None, :], (x.shape[0], n_rx)).copy()
        for a in range(n_tx):
            r -= x[:, a, None] * H[None, :, a]
        d[j0:j0 + x.shape[0]] = np.sum(r.real ** 2 + r.imag ** 2, axis=1)
    jh = int(np.argmin(d))
    dmin = d[jh]
    dsec = np.partition(d, 1)[1] if J > 1 else LD(np.inf)
    gap = float((dsec - dmin) / dmin) if dmin > 0 else float("inf") if dsec > dmin else 0.0
    inv = LD(1) / (LD(varn) * LD(varn))
    z = LD(0)
    m = np.zeros(n_tx, dtype=CLD)
    S = np.zeros((n_tx, n_tx), dtype=CLD)
    for j0 in range(0, J, chunk):
        arg = -(d[j0:min(J, j0 + chunk)] - dmin) * inv
        # exp(arg) is exactly 0 in extended precision below -11400 (its smallest denormal is
        # e^-11399): those hypotheses add exactly nothing and are left out
        sel = np.nonzero(arg > -11500)[0]
        if sel.size == 0:
            continue
        x = c[_hyp(cons, n_tx, j0, min(J, j0 + chunk))[sel]]
        w = np.exp(arg[sel])
        z += w.sum()
        wx = x * w[:, None]
        m += wx.sum(axis=0)
        for a in range(n_tx):
            S[a] += (wx[:, a, None] * np.conj(x)).sum(axis=0)
    xh = np.asarray(cons)[_hyp(cons, n_tx, jh, jh + 1)[0]]
    return dict(m=m / z, S=S / z, mh=xh, Sh=xh[:, None] * np.conj(xh)[None, :], jh=jh, gap=gap)


def moments(theta, y_d, psi_d, cons, varn, n_tx):
    """One trial: y_d (T, n_rx), psi_d (T, P), theta (K,).  Returns dict of complex128 arrays
    m (T, n_tx), S (T, n_tx, n_tx) [soft], mh, Sh [hard], and gap (T,)."""
    y = np.asarray(y_d).astype(CLD)
    T, n_rx = y.shape
    H = heff(theta, psi_d, n_tx, n_rx)
    out = [symbol_moments(H[t], y[t], cons, varn) for t in range(T)]
    res = {k: np.stack([o[k] for o in out]).astype(np.complex128) for k in ("m", "S", "mh", "Sh")}
    res["gap"] = np.array([o["gap"] for o in out])
    return res


def batch_moments(theta, y_d, psi_d, cons, varn, n_tx):
    """moments over a batch: theta (B, K), y_d (B, T, n_rx), psi_d (B, T, P)."""
    per = [moments(theta[i], y_d[i], psi_d[i], cons, varn, n_tx) for i in range(len(y_d))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


# ------------------------------------------------------------------ batch generator
def _cn(g, shape, var=1.0):
    s = np.sqrt(var / 2)
    return g.normal(0, s, shape) + 1j * g.normal(0, s, shape)


def _phases(g, B, T, N):
    psi = np.exp(1j * g.uniform(0, 2 * np.pi, (B, T, N)))
    return np.concatenate([np.ones((B, T, 1), dtype=complex), psi], axis=2)


def synthetic_batch(cons, B, n_tx, n_rx, N, T_d, snr_db, seed, T_p=0):
    """A batch over the table `cons` in the C-ABI layout: theta h is CN(0, 1); psi_d has random
    unit-modulus phases and a direct-path column of ones; symbol indices are uniform over the
    table; y = H_t x + noise of variance varn = E_s / 10^(SNR/10), E_s the table's mean energy.
    theta_wide: an independent CN(0, 1) draw of h's norm (wide posteriors); theta_narrow: h +
    0.05 * a perturbation of unit maximum magnitude.  T_p > 0 adds pilots (y_p, u_p with random
    phases and table symbols) and the least-squares theta0 of the pilots."""
    g = np.random.default_rng(seed)
    cons = np.asarray(cons, dtype=np.complex128)
    M, P = cons.size, N + 1
    K = P * n_tx * n_rx
    varn = float(np.mean(np.abs(cons) ** 2) / 10.0 ** (snr_db / 10.0))
    h = _cn(g, (B, K))
    psi_d = _phases(g, B, T_d, N)
    idx = g.integers(0, M, (B, T_d, n_tx))
    x_d = cons[idx]
    Hm = np.transpose(h.reshape(B, P * n_tx, n_rx), (0, 2, 1))              # (B, n_rx, L)
    u_d = np.einsum("btp,bta->btpa", psi_d, x_d).reshape(B, T_d, P * n_tx)
    y_d = np.einsum("brl,btl->btr", Hm, u_d) + _cn(g, (B, T_d, n_rx), varn)
    wide = _cn(g, (B, K))
    wide *= np.linalg.norm(h, axis=1, keepdims=True) / np.linalg.norm(wide, axis=1, keepdims=True)
    pert = _cn(g, (B, K))
    narrow = h + 0.05 * pert / np.abs(pert).max()
    out = dict(cons=cons, varn=varn, h=h, psi_d=psi_d, x_d=x_d, y_d=y_d, theta_wide=wide,
               theta_narrow=narrow, n_tx=n_tx, n_rx=n_rx, P=P, T_d=T_d, M=M)
    if T_p:
        psi_p = _phases(g, B, T_p, N)
        x_p = cons[g.integers(0, M, (B, T_p, n_tx))]
        u_p = np.einsum("btp,bta->btpa", psi_p, x_p).reshape(B, T_p, P * n_tx)
        y_p = np.einsum("brl,btl->btr", Hm, u_p) + _cn(g, (B, T_p, n_rx), varn)
        H0 = np.einsum("btr,btl->brl", y_p, np.linalg.pinv(np.transpose(u_p, (0, 2, 1))))
        out.update(u_p=u_p, y_p=y_p, theta0=np.transpose(H0, (0, 2, 1)).reshape(B, -1), T_p=T_p)
    return out
