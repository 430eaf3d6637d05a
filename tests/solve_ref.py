"""Inputs with a prescribed spectrum for the M-step's Hermitian solve R X = B^H (csrc/chol.hip and
the solves inside csrc/mstep_small.hip, csrc/mstep_large.hip) and an extended-precision
reference of that solve.

TEST INFRASTRUCTURE ONLY, host only.  np.longdouble / np.clongdouble are x87 extended (64-bit
mantissa, eps = 1.08e-19) on the x86 hosts the suite runs on: 11 bits more than the float64 the
device computes in, so the reference's own error eps_ld cond is 2^-11 of the float64 solve's.

The inputs are legal arguments of sbce.mstep_batch with P = N + 1 phases and T_d = P symbols:

  graded_inputs   psi_d[b] = Q^T with Q a random P x P unitary (column t of Q is psi_t, a
                  different Q per trial), S_t = s_t (I + v_t v_t^H / 2) with s = logspace(0,
                  -decades, P).  The psi_t are orthonormal, so R = sum_t (psi_t psi_t^H) (x) S_t
                  has the eigenvalues of the S_t: s_t (n_tx - 1 times) and s_t (1 + |v_t|^2 / 2),
                  cond_2(R) = 10^decades times a small factor, R dense, B^H dense.
  planted_inputs  the same with Q = I (psi_t = e_t): R is block diagonal with the n_tx x n_tx
                  blocks S_t, the caller gives s_t per trial and block.  The Cholesky pivots of
                  block t are those of S_t alone, whatever the order of the elimination.

Both take the pilots (u_p a Kronecker product, y_p; T_p = 4) from signal_model.synthetic_batch and
scale them down: by sqrt(s_min) 1e-3 (graded: the pilot term is 1e-6 of the smallest eigenvalue)
or by 1e-30 (planted: u_p u_p^H <= 1e-43 of the smallest block, far below its last bit).  A scaled
Kronecker product is still one, so the builds that assume Kronecker pilots stay on their fast path.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)            # 2.22e-16
REL_TOL = 1e-14                                  # the device's pivot threshold, times max diag R
T_P = 4


def _cn(g, shape):
    return (g.standard_normal(shape) + 1j * g.standard_normal(shape)) / np.sqrt(2.0)


def _blocks(g, s, n_tx):
    """S_t = s_t (I + v_t v_t^H / 2), exactly Hermitian with a real diagonal: (..., P, n_tx, n_tx)."""
    v = _cn(g, s.shape + (n_tx,))
    S = s[..., None, None] * (np.eye(n_tx) + 0.5 * v[..., :, None] * np.conj(v[..., None, :]))
    up = np.triu(S, 1)
    return up + np.conj(np.swapaxes(up, -1, -2)) + np.real(S * np.eye(n_tx))


def _inputs(sbce, n_tx, n_rx, N, s, psi_d, pilot_scale, g, seed):
    nb, P = s.shape
    S = _blocks(g, s, n_tx)
    m = np.sqrt(s)[..., None] * _cn(g, (nb, P, n_tx))
    y_d = _cn(g, (nb, P, n_rx))
    b = sbce.signal_model.synthetic_batch(nb, n_tx, n_rx, N, T_P, 1, 4, 0.05, seed=seed)
    return dict(y_d=y_d, y_p=b["y_p"] * pilot_scale, psi_d=psi_d, u_p=b["u_p"] * pilot_scale,
                cons=b["cons"], m=m, S=S, s=s, n_tx=n_tx, n_rx=n_rx, P=P, T_p=T_P, T_d=P,
                L=P * n_tx)


def graded_inputs(sbce, n_tx, n_rx, N, decades, seed, nb):
    """M-step inputs whose R has the spectrum logspace(0, -decades, P) (module docstring)."""
    g = np.random.default_rng(seed)
    P = N + 1
    s = np.tile(np.logspace(0.0, -float(decades), P), (nb, 1))
    Q = np.linalg.qr(_cn(g, (nb, P, P)))[0]
    psi_d = np.ascontiguousarray(np.swapaxes(Q, 1, 2))          # psi_d[b, t, :] = Q[b][:, t]
    return _inputs(sbce, n_tx, n_rx, N, s, psi_d, np.sqrt(s.min()) * 1e-3, g, seed)


def planted_inputs(sbce, n_tx, n_rx, N, s, seed):
    """M-step inputs whose R is block diagonal with blocks S_t of scale s[b, t]: s is (nb, P)."""
    g = np.random.default_rng(seed)
    s = np.asarray(s, dtype=float)
    nb, P = s.shape
    assert P == N + 1
    psi_d = np.tile(np.eye(P, dtype=complex), (nb, 1, 1))
    return _inputs(sbce, n_tx, n_rx, N, s, psi_d, 1e-30, g, seed)


def args_of(inp):
    """The positional arguments of sbce.mstep_batch (varn is not read by the M-step)."""
    return (inp["y_d"], inp["y_p"], inp["psi_d"], inp["u_p"], inp["cons"], inp["m"], inp["S"], 1.0)


def host_system(inp, i):
    """Trial i's R and B^H by the float64 oracle (oracle.em_reduced.mstep_build_gemm)."""
    from oracle.em_reduced import mstep_build_gemm
    return mstep_build_gemm(inp["u_p"][i], inp["y_p"][i], inp["psi_d"][i].T, inp["y_d"][i],
                            inp["m"][i], inp["S"][i])


def herm_lower(R, dtype=CLD):
    """The lower triangle of R completed Hermitian, the diagonal real (some routes return only
    the lower triangle; the device reads no more)."""
    A = np.asarray(R).astype(dtype)
    lo = np.tril(A, -1)
    return lo + np.conj(lo.T) + np.diag(A.diagonal().real).astype(dtype)


def chol_solve_ld(R, rhs, rel_tol=REL_TOL):
    """Unblocked right-looking Cholesky of herm_lower(R) with the forward substitution fused and
    the back substitution after it, all in np.clongdouble, under the device's pivot rule
    (oracle.em_reduced.mstep_chol_policy): a pivot that is not above rel_tol * max diag R is
    dropped -- its column zeroed, its y and x components 0.
    Returns (theta (L n_rx,) clongdouble with theta[l n_rx + r] = conj(X[l, r]), dropped (L,)
    bool, pivots (L,) longdouble: the diagonal entry each column met, before the square root)."""
    A = herm_lower(R)
    L = A.shape[0]
    y = np.array(rhs, dtype=CLD).reshape(L, -1)
    tol = rel_tol * float(A.diagonal().real.max())
    dropped = np.zeros(L, dtype=bool)
    piv = np.zeros(L, dtype=LD)
    for c in range(L):
        d = A[c, c].real
        piv[c] = d
        if not d > tol:
            dropped[c] = True
            A[c:, c] = 0
            y[c] = 0
            continue
        r = np.sqrt(d)
        A[c, c] = r
        col = A[c + 1:, c] / r
        A[c + 1:, c] = col
        y[c] = y[c] / r
        if c + 1 < L:
            A[c + 1:, c + 1:] -= col[:, None] * np.conj(col)[None, :]
            y[c + 1:] -= col[:, None] * y[c][None, :]
    x = np.zeros_like(y)
    for c in range(L - 1, -1, -1):
        if dropped[c]:
            continue
        x[c] = (y[c] - np.conj(A[c + 1:, c]) @ x[c + 1:]) / A[c, c]
    return np.conj(x).reshape(-1), dropped, piv


def backward_error(R, theta, rhs, n_rx):
    """eta = ||R X - B^H||_F / (||R||_F ||X||_F) with X = conj(theta) reshaped (L, n_rx), R
    completed from its lower triangle and the products in long double."""
    A = herm_lower(R)
    L = A.shape[0]
    X = np.conj(np.asarray(theta).astype(CLD)).reshape(L, n_rx)
    res = A @ X - np.asarray(rhs).astype(CLD).reshape(L, n_rx)

    def fro(M):
        return np.sqrt(np.sum(M.real ** 2 + M.imag ** 2))
    return float(fro(res) / (fro(A) * fro(X)))


def rel_ld(a, b):
    """conftest.rel in long double: max |a - b| / max |b|."""
    a = np.asarray(a).astype(CLD).reshape(-1)
    b = np.asarray(b).astype(CLD).reshape(-1)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ the shapes of the GPU tier
# (n_tx, n_rx, N), L = (N + 1) n_tx: the smallest that reach each distinct solve code path
# (launch_mstep_small, launch_chol_batched, launch_chol_large; tests/test_gpu_chol_cond.py)
SHAPES = [
    (2, 2, 15),      # L = 32   small, n_tx <= 2, P <= 16: mstep_small3_solve_kernel (4-column panels)
    (2, 4, 15),      # L = 32   small, same kernels, widest right-hand side
    (1, 4, 12),      # L = 13   small, same kernels, ragged last panel
    (3, 4, 15),      # L = 48   small, mstep_small_kernel, MFMA build
    (3, 2, 20),      # L = 63   small, mstep_small_kernel, VALU build
    (2, 8, 31),      # L = 64   small, mstep_small_kernel, n_rx = 8
    (4, 4, 8),       # L = 36   batched, backsub4, odd 4-column remainder folded
    (4, 1, 16),      # L = 68   batched, backsub4, even 4-column remainder folded
    (3, 4, 22),      # L = 69   batched, backsub4, w = 5, not folded
    (4, 8, 16),      # L = 68   batched, general backsub_kernel, NR = 8
    (4, 4, 28),      # L = 116  batched panel factor, both B-half routes
    (8, 4, 20),      # L = 168  batched panel factor, n_tx = 8, 8-column remainder
    (4, 2, 64),      # L = 260  batched, cfg1's layout; panel_update2_kernel runs
    (4, 2, 74),      # L = 300  batched, L > 272: general back substitution with NR <= 4
    (4, 4, 149),     # L = 600  large, MFMA tile build
    (3, 2, 200),     # L = 603  large, VALU build, partial last tile
]
SEED = 31


def family(shape):
    """The solve family launch_mstep / launch_chol_solve selects by default."""
    n_tx, n_rx, N = shape
    L = (N + 1) * n_tx
    if L > 512:
        return "large"
    return "small" if L <= 64 and n_tx not in (4, 8) else "batched"


def decades_of(shape):
    """At L >= 512 the reference costs seconds: decades 4 and 10 only."""
    return (4, 10) if family(shape) == "large" else (4, 7, 10)


def trials_of(shape):
    return 1 if family(shape) == "large" else 2


def reference(R, rhs, n_rx):
    """What the tests hold a device solve of (R, rhs) against: the long-double solve, cond_2(R),
    and the float64 CPU restatement of the device's policy with its backward error."""
    from oracle.em_reduced import mstep_chol_policy
    R64 = herm_lower(R, np.complex128)
    theta, dropped, piv = chol_solve_ld(R, rhs)
    th_cpu, bad_cpu = mstep_chol_policy(R64, rhs)
    return dict(theta=theta, dropped=dropped, piv=piv, cond=float(np.linalg.cond(R64)),
                tol=REL_TOL * float(R64.diagonal().real.max()), th_cpu=th_cpu, bad_cpu=bad_cpu,
                eta_cpu=backward_error(R, th_cpu, rhs, n_rx))


def forward_bar(cond, three_mfma=False):
    """max(1e-12, 1e-15 cond): the bars of test_gpu_em.py's solve checks; ten times that where the
    complex products are formed from three real MFMAs (the Gauss trick)."""
    return (10.0 if three_mfma else 1.0) * max(1e-12, 1e-15 * cond)


# ------------------------------------------------------------------ planted pivots
S_BIG, S_TINY, S_REST = 1.0, 1e-17, 1e-11


def tiny_positions(shape):
    """{name: block index} of the tiny block's positions: column 0; the block that straddles (or,
    where n_tx divides it, starts at) column 16, 32 and -- on the large route, 64-column tiles --
    64; the block holding the first column of the last 32-column panel (the remainder panel; the
    last 64-column tile on the large route); the last block.  Positions that coincide or do not
    exist at this L are left out."""
    n_tx, n_rx, N = shape
    P, L = N + 1, (N + 1) * n_tx
    tile = 64 if family(shape) == "large" else 32
    want = [("col0", 0)]
    want += [(f"edge{c}", c // n_tx) for c in ((16, 32, 64) if tile == 64 else (16, 32)) if c < L]
    want += [("remainder", (tile * ((L - 1) // tile)) // n_tx), ("last", P - 1)]
    out, seen = {}, set()
    for name, blk in want:
        if blk not in seen:
            seen.add(blk)
            out[name] = blk
    return out


def planted_scales(shape, big, tiny_block):
    """s (2, P): trial 0 has one block at 1 (it holds the largest diagonal entry and so sets tol),
    one at 1e-17 (every pivot of it far below tol) and the rest at 1e-11 (far above); trial 1 is
    the same without the tiny block.  big is "first" or "last"; where the tiny block sits there
    the big one moves to its neighbour.  Returns (s, big_block)."""
    P = shape[2] + 1
    assert P >= 3
    big_block = 0 if big == "first" else P - 1
    if big_block == tiny_block:
        big_block = 1 if big == "first" else P - 2
    s = np.full((2, P), S_REST)
    s[:, big_block] = S_BIG
    s[0, tiny_block] = S_TINY
    return s, big_block


def planted_mask(shape, tiny_block):
    n_tx, n_rx, N = shape
    mask = np.zeros((N + 1) * n_tx, dtype=bool)
    mask[tiny_block * n_tx:(tiny_block + 1) * n_tx] = True
    return mask
