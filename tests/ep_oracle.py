"""Plain NumPy restatement of expectation propagation (include/sbce.h SBCE_ESTEP_EP and
SBCE_LINEAR_EP; csrc/ep_solve.h): per symbol the passes A = G + diag(r) by np.linalg, the cavity
(t, h2), a max-shifted log-sum-exp demapper and the damped state update, in
linear_oracle.linear_ref's style and output keys, plus the per-symbol diagnostics the guards of the
parity cases read.  Also the seeded parity cases, the bound's constant, a 50-digit (mpmath) copy
that fixes it, and the EM chain on linear_em_oracle's batches and M-step.  Test infrastructure
only: the product has no CPU path."""
import functools

import numpy as np

from detect_oracle import bits_of, count_errors, _lse
import linear_em_oracle as eo
import linear_oracle as lo
import noise_oracle as no

EPS = lo.EPS
BETA = 0.5                # damping of the state update          (csrc/ep_solve.h kEpBeta)
VFLOOR = 5e-7             # variance floor, in units of es       (kEpVarFloor)
PASSES = 5                # the default pass count               (kEpDefaultPasses)
B = lo.B

# The parity cases: linear_oracle.SHAPES x VARNS, p = 5.  Seeds are linear_oracle's, except
# (7,8,9,20,64), whose seed there leaves an update 4e-7 from r' = 0 at varn 1.0: it has its own,
# chosen so that every case holds the guards of tests/test_ep.py.
SHAPES, VARNS = lo.SHAPES, lo.VARNS
SEEDS = list(lo.SEEDS)
SEEDS[4] = 2
CASES = [(si, vi) for si in range(len(SHAPES)) for vi in range(len(VARNS))]

# The bound's constant, by linear_oracle's method: R_MEASURED = the largest ratio of |float64
# restatement - 50-digit restatement| to linear_oracle.scales (kappa = the largest cond(A) over the
# passes, x_soft = t and nu = h2 of the last pass) over every parity case and output
# (tests/test_ep.py test_constant_against_extended_precision); 16 = the margin for the device's
# different summation order.  Measured r = 89561 (llr of (4,8,5,16,2) at varn 1.0; x_soft and nu of
# (1,1,1,3,4) at varn 0.3 reach 7.4e4): once a stream is decided the floor makes r_a = s2 / (5e-7 es)
# far larger than G_aa, and mu_a = 1 - r_a g_a = G_aa / (G_aa + r_a) at n_tx = 1 cancels r_a / G_aa
# of its digits whatever cond(A) is (1 for a scalar), so eps cond(A) understates the cavity's error
# by that factor.  post and moments stay below 0.35: a decided stream's posterior does not move.
R_MEASURED = 9.0e4
C_EP = 16.0 * max(R_MEASURED, 1.0)
# The same run, output by output: the cancellation above reaches the cavity (x_soft, nu) and the
# L-values formed from it, while a decided stream's posterior and moments do not move.  The GPU
# tier holds each output to its own constant 16 max(r_k, 1), none above C_EP: 16 for post and the
# moments, which are all the E-step stores.  Measured r_k: x_soft 73655, nu 73630, post 0.344,
# llr 89561, llr_maxlog 89561, moments 0.132.
R_BY_OUTPUT = dict(x_soft=7.4e4, nu=7.4e4, post=0.35, llr=R_MEASURED, llr_maxlog=R_MEASURED,
                   moments=0.14)
C_BY_OUTPUT = {k: 16.0 * max(r, 1.0) for k, r in R_BY_OUTPUT.items()}


def _sigma2(sigma2, Bn):
    return np.broadcast_to(np.asarray(sigma2, dtype=float).reshape(-1), (Bn,)) if np.ndim(sigma2) \
        else np.full(Bn, float(sigma2))


def ep_symbol(H, y, cons, s2, es, passes):
    """The passes of one symbol.  H (n_rx, n_tx), y (n_rx,).  Returns dict(t, h2 (n_tx,), fail,
    kappa, margin_r, margin_v, kept, clamped)."""
    n = H.shape[1]
    G, u = H.conj().T @ H, H.conj().T @ y
    r, q = np.full(n, s2 / es), np.zeros(n, complex)
    o = dict(fail=False, kappa=0.0, margin_r=np.inf, margin_v=np.inf, kept=0, clamped=0)
    c2 = np.abs(cons) ** 2
    for l in range(1, passes + 1):
        A = G + np.diag(r)
        dmax = np.real(np.diag(A)).max()
        try:
            piv = np.real(np.diag(np.linalg.cholesky(A))) ** 2
            fail = bool(np.any(~(piv > 1e-14 * dmax)))
        except np.linalg.LinAlgError:
            fail = True
        if fail:                    # the state no longer changes: every later pass fails alike
            o.update(fail=True, kappa=np.inf, t=np.zeros(n, complex), h2=np.full(n, np.inf))
            return o
        Ai = np.linalg.inv(A)
        g, z = np.real(np.diag(Ai)), Ai @ (u + q)
        o["kappa"] = max(o["kappa"], float(np.linalg.cond(A)))
        mu = 1.0 - r * g
        dead = ~(mu > 0)
        mu = np.where(dead, 1.0, mu)
        t = np.where(dead, 0.0, (z - g * q) / mu)
        h2 = np.where(dead, np.inf, s2 * g / mu)
        o["t"], o["h2"] = t, h2
        if l == passes:
            break
        zz = -np.abs(t[:, None] - cons[None, :]) ** 2 / h2[:, None]
        post = np.exp(zz - _lse(zz, 1)[:, None])
        m, s = post @ cons, post @ c2
        var = s - np.abs(m) ** 2
        floor = VFLOOR * es
        v = np.maximum(var, floor)
        live = ~dead
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            rn = s2 * (1.0 / v - 1.0 / h2)
            qn = s2 * (m / v - t / h2)
            mr = np.abs(1.0 / v - 1.0 / h2) / (1.0 / v + 1.0 / h2)
        if live.any():
            o["margin_r"] = min(o["margin_r"], float(mr[live].min()))
            o["margin_v"] = min(o["margin_v"], float(np.abs(var[live] / floor - 1.0).min()))
        up = live & np.isfinite(rn) & (rn > 0)
        o["kept"] += int((live & ~up).sum())
        o["clamped"] += int((live & (var < floor)).sum())
        r = np.where(up, BETA * rn + (1 - BETA) * r, r)
        q = np.where(up, BETA * qn + (1 - BETA) * q, q)
    return o


def ep_ref(y_d, psi_d, cons, theta, sigma2, n_tx, passes=PASSES, es=None, labels=None,
           x_d_true=None):
    """linear_oracle.linear_ref's arguments and output keys (x_soft = t, nu = h2 of the last pass,
    kappa = the largest cond(A) over the passes), and per symbol margin_r, margin_v (B,T), kept,
    clamped (B,T) int: the updates kept for r' <= 0 and those whose variance met the floor."""
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    Bn, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = max(int(M - 1).bit_length(), 1)
    s2 = _sigma2(sigma2, Bn)
    es = lo.default_es(cons) if es is None else float(es)
    out = dict(x_soft=np.zeros((Bn, T, n_tx), complex), nu=np.zeros((Bn, T, n_tx)),
               idx=np.zeros((Bn, T, n_tx), np.int32), x_hat=np.zeros((Bn, T, n_tx), complex),
               post=np.zeros((Bn, T, n_tx, M)), moments=np.zeros((Bn, T, n_tx + n_tx * n_tx), complex),
               status=np.zeros(Bn, np.int32), fail=np.zeros((Bn, T), bool),
               kappa=np.zeros((Bn, T)), D=np.zeros((Bn, T)), gap=np.zeros((Bn, T, n_tx)),
               margin_r=np.zeros((Bn, T)), margin_v=np.zeros((Bn, T)),
               kept=np.zeros((Bn, T), int), clamped=np.zeros((Bn, T), int))
    bits = None
    if labels is not None:
        bits = bits_of(labels)
        out["llr"] = np.zeros((Bn, T, n_tx, lgM))
        out["llr_maxlog"] = np.zeros((Bn, T, n_tx, lgM))
    for b in range(Bn):
        H = np.einsum("tp,par->tra", psi_d[b], theta[b].reshape(P, n_tx, n_rx))
        for t in range(T):
            e = ep_symbol(H[t], y_d[b, t], cons, s2[b], es, passes)
            for k in ("fail", "kappa", "margin_r", "margin_v", "kept", "clamped"):
                out[k][b, t] = e[k]
            if e["fail"]:
                out["status"][b] |= lo.NONHPD
            xs, nu = e["t"], e["h2"]
            d = np.abs(xs[:, None] - cons[None, :]) ** 2
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


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(si, vi):
    return _frozen(lo.make_case(SHAPES[si], SEEDS[si], VARNS[vi]))


@functools.lru_cache(maxsize=None)
def ref(si, vi, passes=PASSES):
    """The restatement's result of a parity case, computed once and shared (never modified)."""
    c = case(si, vi)
    return _frozen(ep_ref(c["y"], c["psi"], c["cons"], c["theta"], VARNS[vi] ** 2, c["n_tx"],
                          passes=passes, labels=c["labels"], x_d_true=c["x"]))


# linear_oracle.chunk_case() (T_d = 70, three workgroups; trial 1 has two equal channel columns
# from symbol DEFECT_T0 = 40 on) under EP.  A = G + diag(r) with r >= s2 / es stays positive
# definite at the case's own varn = 0.3, so trial 1 alone is given varn = 1e-8: r = 1e-17 then lies
# below the pivot rule's 1e-14 max_a A_aa and exactly the symbols with the planted columns fail, in
# the trial's second and third workgroup.
CHUNK_VARN_T = (lo.CHUNK_VARN, 1e-8, lo.CHUNK_VARN)


@functools.lru_cache(maxsize=None)
def chunk_ref(passes=PASSES):
    c = lo.chunk_case()
    return _frozen(ep_ref(c["y"], c["psi"], c["cons"], c["theta"], np.square(CHUNK_VARN_T),
                          c["n_tx"], passes=passes, labels=c["labels"], x_d_true=c["x"]))


# ------------------------------------------------------------------ extended precision
def ep_ref_mp(y_d, psi_d, cons, theta, sigma2, n_tx, passes, es, labels, digits=50):
    """The same definition in `digits`-digit arithmetic (mpmath), with linear_ref_mp's hand-written
    Cholesky and triangular solves; returns the continuous outputs rounded to float64."""
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
    c2 = [abs(c) ** 2 for c in cm]
    s2, esm = mp.mpf(float(sigma2)), mp.mpf(float(es))
    beta, floor = mp.mpf(BETA), mp.mpf(VFLOOR) * esm
    n = n_tx
    out = dict(x_soft=np.zeros((Bn, T, n), complex), nu=np.zeros((Bn, T, n)),
               post=np.zeros((Bn, T, n, M)), llr=np.zeros((Bn, T, n, lgM)),
               llr_maxlog=np.zeros((Bn, T, n, lgM)), moments=np.zeros((Bn, T, n + n * n), complex))

    def demap(xs, nu):
        d = [abs(xs - c) ** 2 for c in cm]
        zz = [-v / nu for v in d]
        zmax = max(zz)
        ez = [mp.exp(v - zmax) for v in zz]
        tot = sum(ez)
        return zz, ez, [v / tot for v in ez]

    for b in range(Bn):
        th = [[[C_(theta[b, (p * n + a) * n_rx + r]) for r in range(n_rx)] for a in range(n)]
              for p in range(P)]
        for t in range(T):
            ps = [C_(v) for v in psi_d[b, t]]
            H = [[sum(ps[p] * th[p][a][r] for p in range(P)) for a in range(n)] for r in range(n_rx)]
            yv = [C_(v) for v in y_d[b, t]]
            G = [[sum(mp.conj(H[r][i]) * H[r][j] for r in range(n_rx)) for j in range(n)]
                 for i in range(n)]
            u = [sum(mp.conj(H[r][i]) * yv[r] for r in range(n_rx)) for i in range(n)]
            rr, qq = [s2 / esm] * n, [mp.mpc(0)] * n
            for l in range(1, passes + 1):
                A = [[G[i][j] + (rr[i] if i == j else 0) for j in range(n)] for i in range(n)]
                L = [[mp.mpc(0)] * n for _ in range(n)]
                for j in range(n):
                    L[j][j] = mp.sqrt(mp.re(A[j][j] - sum(L[j][k] * mp.conj(L[j][k]) for k in range(j))))
                    for i in range(j + 1, n):
                        L[i][j] = (A[i][j] - sum(L[i][k] * mp.conj(L[j][k]) for k in range(j))) / L[j][j]

                def solve(v):
                    w = [mp.mpc(0)] * n
                    for i in range(n):
                        w[i] = (v[i] - sum(L[i][k] * w[k] for k in range(i))) / L[i][i]
                    x = [mp.mpc(0)] * n
                    for i in reversed(range(n)):
                        x[i] = (w[i] - sum(mp.conj(L[k][i]) * x[k] for k in range(i + 1, n))) / L[i][i]
                    return x

                z = solve([u[i] + qq[i] for i in range(n)])
                g = [mp.re(solve([mp.mpc(1 if i == a else 0) for i in range(n)])[a]) for a in range(n)]
                mu = [1 - rr[a] * g[a] for a in range(n)]
                tt = [(z[a] - g[a] * qq[a]) / mu[a] for a in range(n)]
                h2 = [s2 * g[a] / mu[a] for a in range(n)]
                if l == passes:
                    break
                for a in range(n):
                    _, _, post = demap(tt[a], h2[a])
                    m = sum(p * c for p, c in zip(post, cm))
                    s = sum(p * c for p, c in zip(post, c2))
                    v = max(s - abs(m) ** 2, floor)
                    rn = s2 * (1 / v - 1 / h2[a])
                    qn = s2 * (m / v - tt[a] / h2[a])
                    if rn > 0:
                        rr[a] = beta * rn + (1 - beta) * rr[a]
                        qq[a] = beta * qn + (1 - beta) * qq[a]
            for a in range(n):
                zz, ez, post = demap(tt[a], h2[a])
                out["x_soft"][b, t, a], out["nu"][b, t, a] = complex(tt[a]), float(h2[a])
                out["post"][b, t, a] = [float(v) for v in post]
                for i in range(lgM):
                    s0 = [s for s in range(M) if not bits[s, i]]
                    s1 = [s for s in range(M) if bits[s, i]]
                    out["llr"][b, t, a, i] = float(mp.log(sum(ez[s] for s in s0))
                                                   - mp.log(sum(ez[s] for s in s1)))
                    out["llr_maxlog"][b, t, a, i] = float(max(zz[s] for s in s0)
                                                          - max(zz[s] for s in s1))
                out["moments"][b, t, a] = complex(sum(p * c for p, c in zip(post, cm)))
                out["moments"][b, t, n + a * n + a] = float(sum(p * c for p, c in zip(post, c2)))
            for a in range(n):
                for q in range(n):
                    if a != q:
                        out["moments"][b, t, n + a * n + q] = (out["moments"][b, t, a]
                                                               * np.conj(out["moments"][b, t, q]))
    return out


# ------------------------------------------------------------------ detection cases
# i.i.d. Rayleigh 8 x 8, 16-QAM, sigma2 = the noise the data carry: (SNR dB, seed).  ONE channel
# draw per channel use: P = T_d with one-hot phases psi[t][p] = (t == p), so H_t is block t of
# theta ~ CN(0, 1) -- B T_d = 192 independent 8 x 8 channels and 1536 symbols per case, another
# seed per SNR.  SNR = 10 log10(n_tx es / sigma2) per receive antenna.  The seeds were chosen on
# the CPU so that the restatement meets tests/test_ep.py's condition; test_ep.py prints the counts.
DETECT_SHAPE = (8, 8, 64, 64, 16)
DETECT_CASES = ((16.0, 1), (22.0, 2))


@functools.lru_cache(maxsize=None)
def detect_case(snr_db, seed):
    n_tx, n_rx, P, T_d, M = DETECT_SHAPE
    rs = np.random.RandomState(seed)
    cons, labels = lo.table(M)
    sigma2 = n_tx * lo.default_es(cons) / 10.0 ** (snr_db / 10.0)
    theta = (rs.randn(B, P * n_tx * n_rx) + 1j * rs.randn(B, P * n_tx * n_rx)) / np.sqrt(2)
    psi = np.broadcast_to(np.eye(T_d, P, dtype=complex), (B, T_d, P)).copy()
    x = cons[rs.randint(0, M, size=(B, T_d, n_tx))]
    noise = (rs.randn(B, T_d, n_rx) + 1j * rs.randn(B, T_d, n_rx)) * np.sqrt(sigma2 / 2)
    H = theta.reshape(B, T_d, n_tx, n_rx)                      # H_t[r][a] = theta[(t n_tx + a) n_rx + r]
    y = np.einsum("btar,bta->btr", H, x) + noise
    return _frozen(dict(y=y, psi=psi, cons=cons, labels=labels, theta=theta, x=x, n_tx=n_tx, M=M,
                        sigma2=sigma2))


def symbol_errors(o, c):
    return int(count_errors(o["idx"], c["cons"], c["x"], c["labels"])[:, 0].sum())


# ------------------------------------------------------------------ the EM chain
CHAIN_SHAPES = (eo.S34, eo.S56, eo.S88, eo.S68)
ITERS = eo.ITERS
PERTURB = 1e-13


def estep(c, b, theta, varn, passes=PASSES):
    """(m (T_d, n_tx), S (T_d, n_tx, n_tx), ep_ref's dict) of trial b at theta."""
    n_tx = c["n_tx"]
    o = ep_ref(c["y_d"][b:b + 1], c["psi_d"][b:b + 1], c["cons"], theta[None], varn * varn, n_tx,
               passes=passes)
    mom = o["moments"][0]
    return mom[:, :n_tx], mom[:, n_tx:].reshape(-1, n_tx, n_tx), o


def chain(c, b, iters, theta0=None, varn=None, passes=PASSES):
    """The restated sbce_em (SBCE_ESTEP_EP) of trial b: dict(thetas [theta after each iteration],
    kappa = the largest cond(A) met, fail, margin_r = the smallest met)."""
    theta = np.array(c["theta0"][b] if theta0 is None else theta0, dtype=complex)
    varn = c["varn"] if varn is None else varn
    thetas, kappa, fail, mr = [], 0.0, False, np.inf
    for _ in range(iters):
        m, S, o = estep(c, b, theta, varn, passes)
        kappa, fail = max(kappa, float(o["kappa"].max())), fail or bool(o["fail"].any())
        mr = min(mr, float(o["margin_r"].min()))
        theta = eo.mstep(c, b, m, S)
        thetas.append(theta)
    return dict(thetas=thetas, kappa=kappa, fail=fail, margin_r=mr)


def perturbed(c, b):
    rs = np.random.RandomState(1000 + b)
    th = c["theta0"][b]
    return th * (1 + PERTURB * np.exp(2j * np.pi * rs.rand(th.size)))


@functools.lru_cache(maxsize=None)
def chain_ref(shape, vi=0, iters=ITERS):
    """chain() of every trial of linear_em_oracle.batch(shape, vi), with growth = the factor by
    which a relative 1e-13 perturbation of theta0 grew (the largest over the iterations) and
    bar = 64 eps kappa max(growth, 1), the GPU tier's bound on theta's relative error."""
    c = eo.batch(shape, vi)
    out = []
    for b in range(eo.B):
        r = chain(c, b, iters)
        p = chain(c, b, iters, theta0=perturbed(c, b))
        r["growth"] = max(np.linalg.norm(x - y) / np.linalg.norm(x)
                          for x, y in zip(r["thetas"], p["thetas"])) / PERTURB
        r["fail"], r["margin_r"] = r["fail"] or p["fail"], min(r["margin_r"], p["margin_r"])
        r["kappa"] = max(r["kappa"], p["kappa"])
        r["bar"] = 64.0 * EPS * r["kappa"] * max(r["growth"], 1.0)
        out.append(r)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def noise_chain_ref(shape, vi, iters, start, varn_min=1e-6):
    """The restated sbce_em_noise on the EP E-step, as linear_em_oracle.noise_chain_ref."""
    c = eo.batch(shape, vi)
    out = []
    for b in range(eo.B):
        denom = c["n_rx"] * (c["y_p"].shape[1] + eo.T_D)
        theta, v, status = np.array(c["theta0"][b]), float(start), 0
        hist = np.zeros(iters)
        for l in range(iters):
            m, S, _ = estep(c, b, theta, v)
            theta = eo.mstep(c, b, m, S)
            _, Q, _ = no.noise_var_ref(c["y_d"][b], c["y_p"][b], c["u_p"][b], c["psi_d"][b].T, theta,
                                       m, S, parts=True)
            v, flag = no.apply_rules(Q, denom, v, varn_min)
            status |= flag
            hist[l:] = v
        out.append(dict(theta=theta, varn=v, hist=hist, status=status))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mmse_chain_nmse(shape, vi=0, iters=ITERS):
    """Per-trial NMSE of the MMSE_SOFT chain on the same batch (the yardstick EP is held to)."""
    c = eo.batch(shape, vi)
    return tuple(eo.nmse_of(c, b, r["thetas"][-1]) for b, r in
                 enumerate(eo.chain_ref(shape, vi, "mmse", iters)))
