"""Plain NumPy restatement of linear soft detection (include/sbce.h, sbce_detect_linear): per
symbol A = H^H H + rho I by np.linalg (Cholesky for the pivot rule, inverse for g and z), the
unbiased estimate and its effective noise variance, and a max-shifted log-sum-exp demapper per
stream.  Also the seeded parity cases shared by the CPU and GPU tests, the error bounds, and an
extended-precision (mpmath) copy that fixes the bounds' constant.  Test infrastructure only: the
product has no CPU path."""
import functools

import numpy as np

from detect_oracle import bits_of, count_errors, gray_labeling, _lse

EPS = np.finfo(float).eps
NONHPD = 1

# (n_tx, n_rx, P, T_d, M); B = 3 everywhere
SHAPES = [(1, 1, 1, 3, 4), (2, 2, 3, 5, 16), (3, 8, 33, 18, 4), (5, 6, 3, 17, 16),
          (7, 8, 9, 20, 64), (8, 8, 5, 24, 16), (8, 4, 5, 9, 4), (4, 8, 5, 16, 2)]
VARNS = [0.3, 1.0]
B = 3
# one seed per shape, chosen so that every (b, t) of every (varn, kind) has cond(A) <= 1e4, no
# failed pivot and a relative gap >= 1e-6 between each stream's two nearest table points
# (tests/test_detect_linear.py asserts it)
SEEDS = [1, 1, 1, 2, 1, 133, 1, 1]


def kinds_of(shape):
    return ("mmse", "zf") if shape[1] >= shape[0] else ("mmse",)


CASES = [(si, vi, kind) for si in range(len(SHAPES)) for vi in range(len(VARNS))
         for kind in kinds_of(SHAPES[si])]


def table(M):
    """(cons, labels): the square QAM grid with the reference modem's Gray labelling, or for
    M = 2 a table that is no grid with a labelling that is not the identity."""
    if M == 2:
        return np.array([0.8 + 0.3j, -1.1 - 0.2j]), np.array([1, 0], dtype=np.int32)
    L = int(round(np.sqrt(M)))
    lev = np.arange(-(L - 1), L, 2, dtype=float)
    cons = (lev[:, None] + 1j * lev[None, :]).reshape(-1)
    return cons, gray_labeling(M)


def make_case(shape, seed, varn):
    """Data drawn from the model at noise sigma2 = varn^2: theta ~ CN(0, 1/P) (so H_t ~ CN(0, 1)
    under unit-modulus phases), uniform symbols, y = H_t x + CN(0, sigma2)."""
    n_tx, n_rx, P, T_d, M = shape
    rs = np.random.RandomState(seed)
    cons, labels = table(M)
    theta = (rs.randn(B, P * n_tx * n_rx) + 1j * rs.randn(B, P * n_tx * n_rx)) / np.sqrt(2 * P)
    psi = np.exp(2j * np.pi * rs.rand(B, T_d, P))
    ix = rs.randint(0, M, size=(B, T_d, n_tx))
    x = cons[ix]
    noise = (rs.randn(B, T_d, n_rx) + 1j * rs.randn(B, T_d, n_rx)) * np.sqrt(varn * varn / 2)
    H = np.einsum("btp,bpar->btra", psi, theta.reshape(B, P, n_tx, n_rx))
    y = np.einsum("btra,bta->btr", H, x) + noise
    return dict(y=y, psi=psi, cons=cons, labels=labels, theta=theta, x=x, n_tx=n_tx, M=M)


def default_es(cons):
    return float(np.mean(np.abs(np.asarray(cons)) ** 2))


def linear_ref(y_d, psi_d, cons, theta, sigma2, n_tx, kind="mmse", es=None, labels=None,
               x_d_true=None):
    """y_d (B,T,n_rx), psi_d (B,T,P), cons (M,), theta (B,K), sigma2 scalar or (B,).
    Returns dict(x_soft, nu (B,T,n_tx), idx int32, x_hat, post (B,T,n_tx,M), moments
    (B,T,n_tx+n_tx^2), status (B,) int32, fail (B,T) bool, kappa (B,T) = cond(A), D (B,T) =
    max_{a,s} d, gap (B,T,n_tx) = relative gap of each stream's two smallest d [, llr, llr_maxlog
    with labels] [, err with x_d_true and labels])."""
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    Bn, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = max(int(M - 1).bit_length(), 1)
    s2 = np.broadcast_to(np.asarray(sigma2, dtype=float).reshape(-1), (Bn,)) if np.ndim(sigma2) \
        else np.full(Bn, float(sigma2))
    es = default_es(cons) if es is None else float(es)
    out = dict(x_soft=np.zeros((Bn, T, n_tx), complex), nu=np.zeros((Bn, T, n_tx)),
               idx=np.zeros((Bn, T, n_tx), np.int32), x_hat=np.zeros((Bn, T, n_tx), complex),
               post=np.zeros((Bn, T, n_tx, M)), moments=np.zeros((Bn, T, n_tx + n_tx * n_tx), complex),
               status=np.zeros(Bn, np.int32), fail=np.zeros((Bn, T), bool),
               kappa=np.zeros((Bn, T)), D=np.zeros((Bn, T)), gap=np.zeros((Bn, T, n_tx)))
    bits = None
    if labels is not None:
        bits = bits_of(labels)
        out["llr"] = np.zeros((Bn, T, n_tx, lgM))
        out["llr_maxlog"] = np.zeros((Bn, T, n_tx, lgM))
    for b in range(Bn):
        rho = s2[b] / es if kind == "mmse" else 0.0
        H = np.einsum("tp,par->tra", psi_d[b], theta[b].reshape(P, n_tx, n_rx))
        for t in range(T):
            A = H[t].conj().T @ H[t] + rho * np.eye(n_tx)
            dmax = np.real(np.diag(A)).max()
            try:
                piv = np.real(np.diag(np.linalg.cholesky(A))) ** 2
                fail = bool(np.any(~(piv > 1e-14 * dmax)))
            except np.linalg.LinAlgError:
                fail = True
            if fail:
                xs, nu = np.zeros(n_tx, complex), np.full(n_tx, np.inf)
                out["fail"][b, t] = True
                out["status"][b] |= NONHPD
                out["kappa"][b, t] = np.inf
            else:
                Ai = np.linalg.inv(A)
                g = np.real(np.diag(Ai))
                z = Ai @ (H[t].conj().T @ y_d[b, t])
                out["kappa"][b, t] = np.linalg.cond(A)
                if kind == "mmse":
                    mu = 1.0 - rho * g
                    dead = ~(mu > 0)                      # a zero channel column
                    mu = np.where(dead, 1.0, mu)
                    xs = np.where(dead, 0.0, z / mu)
                    nu = np.where(dead, np.inf, es * (rho * g) / mu)   # es (1 - mu) / mu
                else:
                    xs, nu = z, s2[b] * g
            d = np.abs(xs[:, None] - cons[None, :]) ** 2          # (n_tx, M)
            zz = -d / nu[:, None]
            post = np.exp(zz - _lse(zz, 1)[:, None])
            idx = np.argmin(d, axis=1)
            two = np.sort(d, axis=1)[:, :2]
            out["gap"][b, t] = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
            out["D"][b, t] = d.max()
            out["x_soft"][b, t], out["nu"][b, t] = xs, nu
            out["idx"][b, t], out["x_hat"][b, t], out["post"][b, t] = idx, cons[idx], post
            m = post @ cons
            S = np.outer(m, m.conj())
            S[np.arange(n_tx), np.arange(n_tx)] = post @ (np.abs(cons) ** 2)
            out["moments"][b, t] = np.concatenate([m, S.reshape(-1)])
            if bits is not None:
                for i in range(lgM):
                    one = bits[:, i] == 1
                    out["llr"][b, t, :, i] = _lse(zz[:, ~one], 1) - _lse(zz[:, one], 1)
                    out["llr_maxlog"][b, t, :, i] = (d[:, one].min(axis=1)
                                                     - d[:, ~one].min(axis=1)) / nu
    if x_d_true is not None and labels is not None:
        out["err"] = count_errors(out["idx"], cons, x_d_true, labels)
    return out


def oracle_detect_linear_batch(y_d, psi_d, cons, theta, varn, n_tx, kind="mmse", es=None,
                               labels=None, x_d_true=None, noise="em", maxlog=False, want=(),
                               return_device=False):
    """detect_linear_batch's contract computed by the restatement (the sweep only reads 'err')."""
    v = np.asarray(varn, dtype=float)
    r = linear_ref(y_d, psi_d, cons, theta, v * v if noise == "em" else v, n_tx, kind=kind, es=es,
                   labels=labels, x_d_true=x_d_true)
    return {"err": r["err"]}


@functools.lru_cache(maxsize=None)
def case(si, vi):
    c = make_case(SHAPES[si], SEEDS[si], VARNS[vi])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref(si, vi, kind):
    """The restatement's result of a parity case, computed once and shared (never modified)."""
    c = case(si, vi)
    r = linear_ref(c["y"], c["psi"], c["cons"], c["theta"], VARNS[vi] ** 2, c["n_tx"], kind=kind,
                   labels=c["labels"], x_d_true=c["x"])
    for v in r.values():
        v.setflags(write=False)
    return r


# ------------------------------------------------------------------ bounds
# The error of a Cholesky solve scales with eps cond(A); a demapper argument d / nu of size up to
# D / nu turns a relative error into an absolute one of that size.  C is fixed on the CPU by
# tests/test_detect_linear.py (test_constant_against_extended_precision): r = the largest ratio of
# |float64 restatement - 50-digit restatement| to the scales below over every parity case and
# output, C = 16 max(r, 1).  Measured r = 17.65: x_soft of the MMSE case (8,4,5,9,4) at varn 0.3,
# where n_rx < n_tx leaves weak directions with mu = 1 - rho g close to 0, so that the division
# by mu amplifies g's own eps kappa error once more.  Every other case and output stays below 4.
R_MEASURED = 17.65
C = 16.0 * max(R_MEASURED, 1.0)


def scales(o, cons):
    """eps kappa_t scale per output of a restatement result `o` (C not applied): dict of arrays
    broadcastable against the outputs.  moments: term s of m_a = sum_s post_s cons_s carries the
    posterior's bound times |cons_s|, so m_a gets sum_s |cons_s| times it and S[a][a] gets
    sum_s |cons_s|^2 times it; S[a][c] = m_a conj(m_c) gets |m_a| bound(m_c) + |m_c| bound(m_a)
    with |m| <= max |cons|."""
    k = EPS * o["kappa"][:, :, None]
    with np.errstate(invalid="ignore"):
        dn = 1.0 + o["D"][:, :, None] / o["nu"]
    pb = k * dn
    ac = np.abs(np.asarray(cons))
    n_tx = o["nu"].shape[2]
    mb = ac.sum() * pb                                      # (B,T,n_tx): m_a
    Sb = float(ac.max()) * (mb[:, :, :, None] + mb[:, :, None, :])
    i = np.arange(n_tx)
    Sb[:, :, i, i] = (ac ** 2).sum() * pb
    return dict(x_soft=k * (1.0 + np.abs(o["x_soft"])), nu=k * o["nu"], post=pb[..., None],
                llr=pb[..., None], llr_maxlog=pb[..., None],
                moments=np.concatenate([mb, Sb.reshape(Sb.shape[0], Sb.shape[1], -1)], axis=2))


def ratios(got, o, cons, ok=None):
    """max over each output of |got - o| / (eps kappa scale); `got` uses the restatement's keys.
    ok (B,T) bool: the symbols that count (a failed symbol has kappa = nu = inf: its outputs are
    compared exactly by the caller)."""
    with np.errstate(invalid="ignore"):
        sc = scales(o, cons)
        out = {}
        for k in sc:
            if k in got:
                r = np.abs(np.asarray(got[k]) - o[k]) / sc[k]
                out[k] = float(np.max(r if ok is None else r[ok]))
    return out


# ------------------------------------------------------------------ several workgroups per trial
# The device kernel takes 32 symbols per workgroup, so the listed parity shapes (T_d <= 24) run one
# workgroup per trial.  This case has T_d = 70 (two full chunks and a ragged one of 6) and, in
# trial 1 only, a defect that starts in the second chunk: streams 1 and 3 share their theta rows
# of p = 1 and the phase of p = 0 is zero from symbol DEFECT_T0 on, so H_t has two equal columns
# there and ZF's A is singular -- the status flag comes from workgroups other than the first.
CHUNK_SHAPE, CHUNK_SEED, CHUNK_VARN, DEFECT_T0 = (5, 6, 2, 70, 16), 1, 0.3, 40


@functools.lru_cache(maxsize=None)
def chunk_case():
    c = make_case(CHUNK_SHAPE, CHUNK_SEED, CHUNK_VARN)
    n_tx, n_rx, P, T_d, M = CHUNK_SHAPE
    th = c["theta"].reshape(B, P, n_tx, n_rx).copy()
    th[1, 1, 3, :] = th[1, 1, 1, :]
    psi = c["psi"].copy()
    psi[1, DEFECT_T0:, 0] = 0.0
    c["theta"], c["psi"] = th.reshape(B, -1), psi
    H = np.einsum("btp,bpar->btra", psi, th)
    rs = np.random.RandomState(CHUNK_SEED + 1000)
    noise = (rs.randn(B, T_d, n_rx) + 1j * rs.randn(B, T_d, n_rx)) * np.sqrt(CHUNK_VARN ** 2 / 2)
    c["y"] = np.einsum("btra,bta->btr", H, c["x"]) + noise
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def chunk_ref(kind):
    c = chunk_case()
    r = linear_ref(c["y"], c["psi"], c["cons"], c["theta"], CHUNK_VARN ** 2, c["n_tx"], kind=kind,
                   labels=c["labels"], x_d_true=c["x"])
    for v in r.values():
        v.setflags(write=False)
    return r


# ------------------------------------------------------------------ extended precision
def linear_ref_mp(y_d, psi_d, cons, theta, sigma2, n_tx, kind, es, labels, digits=50):
    """The same definition in `digits`-digit arithmetic (mpmath), with a hand-written Cholesky
    (at most 8 x 8) and triangular solves; returns the continuous outputs rounded to float64."""
    import mpmath as mp
    mp.mp.dps = digits
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    Bn, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = max(int(M - 1).bit_length(), 1)
    bits = bits_of(labels)
    C_ = lambda v: mp.mpc(float(np.real(v)), float(np.imag(v)))
    cm = [C_(c) for c in cons]
    s2, esm = mp.mpf(float(sigma2)), mp.mpf(float(es))
    rho = s2 / esm if kind == "mmse" else mp.mpf(0)
    n = n_tx
    out = dict(x_soft=np.zeros((Bn, T, n), complex), nu=np.zeros((Bn, T, n)),
               post=np.zeros((Bn, T, n, M)), llr=np.zeros((Bn, T, n, lgM)),
               llr_maxlog=np.zeros((Bn, T, n, lgM)), moments=np.zeros((Bn, T, n + n * n), complex))

    for b in range(Bn):
        th = [[[C_(theta[b, (p * n + a) * n_rx + r]) for r in range(n_rx)] for a in range(n)]
              for p in range(P)]
        for t in range(T):
            ps = [C_(v) for v in psi_d[b, t]]
            H = [[sum(ps[p] * th[p][a][r] for p in range(P)) for a in range(n)] for r in range(n_rx)]
            yv = [C_(v) for v in y_d[b, t]]
            A = [[sum(mp.conj(H[r][i]) * H[r][j] for r in range(n_rx)) + (rho if i == j else 0)
                  for j in range(n)] for i in range(n)]
            rhs = [sum(mp.conj(H[r][i]) * yv[r] for r in range(n_rx)) for i in range(n)]
            L = [[mp.mpc(0)] * n for _ in range(n)]
            for j in range(n):
                L[j][j] = mp.sqrt(mp.re(A[j][j] - sum(L[j][k] * mp.conj(L[j][k]) for k in range(j))))
                for i in range(j + 1, n):
                    L[i][j] = (A[i][j] - sum(L[i][k] * mp.conj(L[j][k]) for k in range(j))) / L[j][j]

            def solve(v):                                    # A^-1 v = L^-H L^-1 v
                u = [mp.mpc(0)] * n
                for i in range(n):
                    u[i] = (v[i] - sum(L[i][k] * u[k] for k in range(i))) / L[i][i]
                x = [mp.mpc(0)] * n
                for i in reversed(range(n)):
                    x[i] = (u[i] - sum(mp.conj(L[k][i]) * x[k] for k in range(i + 1, n))) / L[i][i]
                return x

            z = solve(rhs)
            g = [mp.re(solve([mp.mpc(1 if i == a else 0) for i in range(n)])[a]) for a in range(n)]
            for a in range(n):
                if kind == "mmse":
                    mu = 1 - rho * g[a]
                    xs, nu = z[a] / mu, esm * (1 - mu) / mu
                else:
                    xs, nu = z[a], s2 * g[a]
                d = [abs(xs - c) ** 2 for c in cm]
                zz = [-v / nu for v in d]
                zmax = max(zz)
                ez = [mp.exp(v - zmax) for v in zz]          # mpmath's exponent never underflows
                tot = sum(ez)
                post = [v / tot for v in ez]
                out["x_soft"][b, t, a], out["nu"][b, t, a] = complex(xs), float(nu)
                out["post"][b, t, a] = [float(v) for v in post]
                for i in range(lgM):
                    s0 = [s for s in range(M) if not bits[s, i]]
                    s1 = [s for s in range(M) if bits[s, i]]
                    out["llr"][b, t, a, i] = float(mp.log(sum(ez[s] for s in s0))
                                                   - mp.log(sum(ez[s] for s in s1)))
                    out["llr_maxlog"][b, t, a, i] = float(max(zz[s] for s in s0)
                                                          - max(zz[s] for s in s1))
                out["moments"][b, t, a] = complex(sum(p * c for p, c in zip(post, cm)))
                out["moments"][b, t, n + a * n + a] = float(sum(p * abs(c) ** 2 for p, c in zip(post, cm)))
            for a in range(n):
                for q in range(n):
                    if a != q:
                        out["moments"][b, t, n + a * n + q] = (out["moments"][b, t, a]
                                                               * np.conj(out["moments"][b, t, q]))
    return out
