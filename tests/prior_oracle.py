"""Plain NumPy restatement of soft-input expectation propagation (include/sbce.h
sbce_detect_linear_prior / sbce_estep_prior / sbce_em_prior; csrc/ep_prior.h): ep_oracle's passes
started from the moments of the a-priori pmf, with a prior-weighted max-shifted log-sum-exp
demapper, in ep_oracle.ep_ref's style and output keys.  Also the seeded parity cases, their error
scales, a 50-digit (mpmath) copy that fixes the bound's constants, and the EM chain on
linear_em_oracle's batches.  Test infrastructure only: the product has no CPU path."""
import functools
import importlib

import numpy as np

from conftest import PKG
from detect_oracle import bits_of, count_errors, _lse
import ep_oracle as ep
import linear_em_oracle as eo
import linear_oracle as lo
import noise_oracle as no

qam = importlib.import_module(PKG + ".qam")

EPS = lo.EPS
CLAMP = 64.0              # |La| after the load                   (csrc/ep_prior.h kPriorClamp)
BETA, VFLOOR = ep.BETA, ep.VFLOOR
B = lo.B

# The parity cases: linear_oracle.SHAPES x VARNS x I_A x p.  la = prior_llr_gaussian at I_A on
# the true bits (seed 5000 + the case's own), with four planted entries: +inf, -inf, NaN and 1e3.
SHAPES, VARNS = lo.SHAPES, lo.VARNS
IAS = (0.3, 0.8)
PASSES = (1, 5)
# one seed per shape, chosen so that every case holds the guards of tests/test_prior.py
SEEDS = list(lo.SEEDS)
# the seed of a case's L-values is 5000 + 100 si + 10 vi + ii, except where that draw leaves a
# posterior variance within 1e-3 of its floor at p = 5 (as ep_oracle gives shape 4 its own seed)
LA_SEEDS = {(5, 1, 1): 1}
CASES = [(si, vi, ii) for si in range(len(SHAPES)) for vi in range(len(VARNS))
         for ii in range(len(IAS))]
GAP = 1e-6                # relative MAP-decision gap below which idx_hat is not compared

# The bounds' constants, by ep_oracle's method: r_k = the largest ratio of |float64 restatement -
# 50-digit restatement| to scales() over every parity case (both pass counts), output by output;
# C_k = 16 max(r_k, 1), 16 being the margin for the device's different summation order.  Measured
# by tests/test_prior.py test_constants_against_extended_precision (which prints them); they are
# not ep_oracle's: a strong prior floors v0 from pass 1 on, so the cancellation of
# mu_a = 1 - r_a g_a is met in the first pass already.
# Measured r_k: x_soft 85090 ((4,8,5,16,2) varn 1.0 I_A 0.3 p 5), nu 146531 ((1,1,1,3,4) varn 1.0
# I_A 0.8 p 5), post 0.632, llr 49147, llr_maxlog 49147, moments 0.212 (post and moments:
# (8,4,5,9,4) varn 0.3 I_A 0.3 p 1).  As in ep_oracle the cavity of a decided stream cancels
# r_a / G_aa of its digits whatever cond(A) is, while its posterior and moments do not move.
R_BY_OUTPUT = dict(x_soft=8.6e4, nu=1.5e5, post=0.64, llr=5.0e4, llr_maxlog=5.0e4, moments=0.22)
C_BY_OUTPUT = {k: 16.0 * max(r, 1.0) for k, r in R_BY_OUTPUT.items()}


def sanitise(la):
    la = np.array(la, dtype=float)
    la[np.isnan(la)] = 0.0
    return np.clip(la, -CLAMP, CLAMP)


def prior_lp(la, bits):
    """la (n, lgM) sanitised, bits (M, lgM): lp (n, M) = -sum_i bit_i(s) La_i, largest member 0."""
    lp = -(la[:, None, :] * bits[None, :, :]).sum(axis=2)
    return lp - lp.max(axis=1, keepdims=True)


def _softmax(zz):
    return np.exp(zz - _lse(zz, 1)[:, None])


def ep_prior_symbol(H, y, cons, lp, s2, es, passes):
    """The passes of one symbol from the prior lp (n_tx, M).  Returns ep_oracle.ep_symbol's dict
    (a failed symbol: t = 0, h2 = inf) plus dead (n_tx,) of the last pass and kappa0 =
    cond(G + (s2 / es) I), the conditioning of the channel itself (the prior-free first pass)."""
    n = H.shape[1]
    G, u = H.conj().T @ H, H.conj().T @ y
    c2 = np.abs(cons) ** 2
    floor = VFLOOR * es
    pi = _softmax(lp)
    xbar = pi @ cons
    v0 = np.maximum(pi @ c2 - np.abs(xbar) ** 2, floor)
    r, q = s2 / v0, s2 * xbar / v0
    o = dict(fail=False, kappa=0.0, margin_r=np.inf, margin_v=np.inf, kept=0, clamped=0,
             kappa0=float(np.linalg.cond(G + (s2 / es) * np.eye(n))))
    for l in range(1, passes + 1):
        A = G + np.diag(r)
        dmax = np.real(np.diag(A)).max()
        try:
            piv = np.real(np.diag(np.linalg.cholesky(A))) ** 2
            fail = bool(np.any(~(piv > 1e-14 * dmax)))
        except np.linalg.LinAlgError:
            fail = True
        if fail:
            o.update(fail=True, kappa=np.inf, t=np.zeros(n, complex), h2=np.full(n, np.inf),
                     dead=np.ones(n, bool))
            return o
        Ai = np.linalg.inv(A)
        g, z = np.real(np.diag(Ai)), Ai @ (u + q)
        o["kappa"] = max(o["kappa"], float(np.linalg.cond(A)))
        mu = 1.0 - r * g
        dead = ~(mu > 0)
        mu = np.where(dead, 1.0, mu)
        t = np.where(dead, 0.0, (z - g * q) / mu)
        h2 = np.where(dead, np.inf, s2 * g / mu)
        o["t"], o["h2"], o["dead"] = t, h2, dead
        if l == passes:
            break
        post = _softmax(-np.abs(t[:, None] - cons[None, :]) ** 2 / h2[:, None] + lp)
        m, s = post @ cons, post @ c2
        var = s - np.abs(m) ** 2
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


def ep_prior_ref(y_d, psi_d, cons, theta, sigma2, n_tx, la, passes=ep.PASSES, es=None, labels=None,
                 x_d_true=None):
    """ep_oracle.ep_ref's arguments and keys plus la (B,T,n_tx,lgM) (raw: sanitised here; labels
    are required).  x_soft = t, nu = h2 (extrinsic), post / moments / idx / x_hat a-posteriori,
    llr and llr_maxlog extrinsic (L_post - La); gap = the relative gap of each stream's two largest
    exponents -d_s / h2 + lp[s]; D = the largest |exponent| argument scale (see scales)."""
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    Bn, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = max(int(M - 1).bit_length(), 1)
    s2 = ep._sigma2(sigma2, Bn)
    es = lo.default_es(cons) if es is None else float(es)
    bits = bits_of(labels)
    la = sanitise(la).reshape(Bn, T, n_tx, lgM)
    out = dict(x_soft=np.zeros((Bn, T, n_tx), complex), nu=np.zeros((Bn, T, n_tx)),
               idx=np.zeros((Bn, T, n_tx), np.int32), x_hat=np.zeros((Bn, T, n_tx), complex),
               post=np.zeros((Bn, T, n_tx, M)), moments=np.zeros((Bn, T, n_tx + n_tx * n_tx), complex),
               status=np.zeros(Bn, np.int32), fail=np.zeros((Bn, T), bool),
               dead=np.zeros((Bn, T, n_tx), bool), prior=np.zeros((Bn, T, n_tx, M)),
               kappa=np.zeros((Bn, T)), D=np.zeros((Bn, T)), gap=np.zeros((Bn, T, n_tx)),
               E=np.zeros((Bn, T, n_tx)), kappa0=np.zeros((Bn, T)),
               margin_r=np.zeros((Bn, T)), margin_v=np.zeros((Bn, T)),
               kept=np.zeros((Bn, T), int), clamped=np.zeros((Bn, T), int), la=la,
               llr=np.zeros((Bn, T, n_tx, lgM)), llr_maxlog=np.zeros((Bn, T, n_tx, lgM)))
    for b in range(Bn):
        H = np.einsum("tp,par->tra", psi_d[b], theta[b].reshape(P, n_tx, n_rx))
        for t in range(T):
            lp = prior_lp(la[b, t], bits)
            e = ep_prior_symbol(H[t], y_d[b, t], cons, lp, s2[b], es, passes)
            for k in ("fail", "kappa", "kappa0", "margin_r", "margin_v", "kept", "clamped", "dead"):
                out[k][b, t] = e[k]
            if e["fail"]:
                out["status"][b] |= lo.NONHPD
            xs, nu = e["t"], e["h2"]
            d = np.abs(xs[:, None] - cons[None, :]) ** 2
            zz = -d / nu[:, None] + lp
            post = _softmax(zz)
            idx = np.argmax(zz, axis=1)
            two = np.sort(zz, axis=1)[:, ::-1][:, :2]
            out["gap"][b, t] = (two[:, 0] - two[:, 1]) / np.maximum(np.abs(two).max(axis=1), 1e-300)
            out["D"][b, t] = d.max()
            out["E"][b, t] = np.abs(zz).max(axis=1)          # the largest |exponent| of the stream
            out["prior"][b, t] = _softmax(lp)
            out["x_soft"][b, t], out["nu"][b, t] = xs, nu
            out["idx"][b, t], out["x_hat"][b, t], out["post"][b, t] = idx, cons[idx], post
            m = post @ cons
            S = np.outer(m, m.conj())
            S[np.arange(n_tx), np.arange(n_tx)] = post @ (np.abs(cons) ** 2)
            out["moments"][b, t] = np.concatenate([m, S.reshape(-1)])
            for i in range(lgM):
                one = bits[:, i] == 1
                ex = _lse(zz[:, ~one], 1) - _lse(zz[:, one], 1) - la[b, t, :, i]
                ml = zz[:, ~one].max(axis=1) - zz[:, one].max(axis=1) - la[b, t, :, i]
                out["llr"][b, t, :, i] = np.where(e["dead"], 0.0, ex)
                out["llr_maxlog"][b, t, :, i] = np.where(e["dead"], 0.0, ml)
    if x_d_true is not None:
        out["err"] = count_errors(out["idx"], cons, x_d_true, labels)
    return out


def scales(o, cons):
    """linear_oracle.scales with the demapper's argument scale taken from the prior-weighted
    exponents: a relative error eps kappa of (t, h2) moves an exponent -d / h2 + lp by at most
    eps kappa (1 + D / h2), and forming lp (<= 6 terms of size <= 64) adds eps |lp|, which
    E = max_s |exponent| covers together with the shift."""
    k = EPS * o["kappa"][:, :, None]
    with np.errstate(invalid="ignore"):
        dn = 1.0 + o["D"][:, :, None] / o["nu"] + o["E"]
    pb = k * dn
    ac = np.abs(np.asarray(cons))
    n_tx = o["nu"].shape[2]
    mb = ac.sum() * pb
    Sb = float(ac.max()) * (mb[:, :, :, None] + mb[:, :, None, :])
    i = np.arange(n_tx)
    Sb[:, :, i, i] = (ac ** 2).sum() * pb
    return dict(x_soft=k * (1.0 + np.abs(o["x_soft"])), nu=k * o["nu"], post=pb[..., None],
                llr=pb[..., None], llr_maxlog=pb[..., None],
                moments=np.concatenate([mb, Sb.reshape(Sb.shape[0], Sb.shape[1], -1)], axis=2))


def ratios(got, o, cons, ok=None):
    """max over each output of |got - o| / scale; ok (B,T) bool: the symbols that count."""
    with np.errstate(invalid="ignore"):
        sc = scales(o, cons)
        out = {}
        for k in sc:
            if k in got:
                r = np.abs(np.asarray(got[k]) - o[k]) / sc[k]
                out[k] = float(np.max(r if ok is None else r[ok]))
    return out


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def true_bits(x, cons, labels):
    idx = np.argmin(np.abs(np.asarray(x)[..., None] - np.asarray(cons)), axis=-1)
    return bits_of(labels)[idx]


def planted(la):
    """The four planted entries of a case: +inf, -inf, NaN, 1e3 at fixed flat positions."""
    flat = la.reshape(-1)
    n = flat.size
    for pos, v in zip((0, n // 3, n // 2, n - 1), (np.inf, -np.inf, np.nan, 1e3)):
        flat[pos] = v
    return la


@functools.lru_cache(maxsize=None)
def case(si, vi, ii):
    c = dict(lo.make_case(SHAPES[si], SEEDS[si], VARNS[vi]))
    rs = np.random.RandomState(LA_SEEDS.get((si, vi, ii), 5000 + 100 * si + 10 * vi + ii))
    c["la"] = planted(qam.prior_llr_gaussian(true_bits(c["x"], c["cons"], c["labels"]), IAS[ii], rs))
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def ref(si, vi, ii, passes):
    c = case(si, vi, ii)
    return _frozen(ep_prior_ref(c["y"], c["psi"], c["cons"], c["theta"], VARNS[vi] ** 2, c["n_tx"],
                                c["la"], passes=passes, labels=c["labels"], x_d_true=c["x"]))


# linear_oracle.chunk_case() under ep_oracle.CHUNK_VARN_T (trial 1 at varn 1e-8 with planted equal
# columns from DEFECT_T0 on) with moderate priors |La| <= 4 on every trial.
@functools.lru_cache(maxsize=None)
def chunk_la():
    c = lo.chunk_case()
    rs = np.random.RandomState(77)
    la = qam.prior_llr_gaussian(true_bits(c["x"], c["cons"], c["labels"]), 0.3, rs)
    la = np.clip(la, -4.0, 4.0)
    la.setflags(write=False)
    return la


@functools.lru_cache(maxsize=None)
def chunk_ref(passes=ep.PASSES):
    c = lo.chunk_case()
    return _frozen(ep_prior_ref(c["y"], c["psi"], c["cons"], c["theta"], np.square(ep.CHUNK_VARN_T),
                                c["n_tx"], chunk_la(), passes=passes, labels=c["labels"],
                                x_d_true=c["x"]))


# ------------------------------------------------------------------ extended precision
def ep_prior_ref_mp(y_d, psi_d, cons, theta, sigma2, n_tx, la, passes, es, labels, digits=50):
    """The same definition in `digits`-digit arithmetic (mpmath), with ep_oracle.ep_ref_mp's
    hand-written Cholesky and triangular solves; the continuous outputs rounded to float64."""
    import mpmath as mp
    mp.mp.dps = digits
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    Bn, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = max(int(M - 1).bit_length(), 1)
    bits = bits_of(labels)
    la = sanitise(la).reshape(Bn, T, n_tx, lgM)
    C_ = lambda v: mp.mpc(float(np.real(v)), float(np.imag(v)))
    cm = [C_(c) for c in cons]
    c2 = [abs(c) ** 2 for c in cm]
    s2, esm = mp.mpf(float(sigma2)), mp.mpf(float(es))
    beta, floor = mp.mpf(BETA), mp.mpf(VFLOOR) * esm
    n = n_tx
    out = dict(x_soft=np.zeros((Bn, T, n), complex), nu=np.zeros((Bn, T, n)),
               post=np.zeros((Bn, T, n, M)), llr=np.zeros((Bn, T, n, lgM)),
               llr_maxlog=np.zeros((Bn, T, n, lgM)), moments=np.zeros((Bn, T, n + n * n), complex))

    def demap(xs, inv, lp):
        zz = [-abs(xs - c) ** 2 * inv + l for c, l in zip(cm, lp)]
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
            lps = []
            for a in range(n):
                raw = [-sum(mp.mpf(float(la[b, t, a, i])) for i in range(lgM) if bits[s, i])
                       for s in range(M)]
                top = max(raw)
                lps.append([v - top for v in raw])
            rr, qq = [], []
            for a in range(n):
                _, _, pi = demap(mp.mpc(0), mp.mpf(0), lps[a])
                xbar = sum(p * c for p, c in zip(pi, cm))
                v0 = max(sum(p * c for p, c in zip(pi, c2)) - abs(xbar) ** 2, floor)
                rr.append(s2 / v0)
                qq.append(s2 * xbar / v0)
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
                    _, _, post = demap(tt[a], 1 / h2[a], lps[a])
                    m = sum(p * c for p, c in zip(post, cm))
                    s = sum(p * c for p, c in zip(post, c2))
                    v = max(s - abs(m) ** 2, floor)
                    rn = s2 * (1 / v - 1 / h2[a])
                    qn = s2 * (m / v - tt[a] / h2[a])
                    if rn > 0:
                        rr[a] = beta * rn + (1 - beta) * rr[a]
                        qq[a] = beta * qn + (1 - beta) * qq[a]
            for a in range(n):
                zz, ez, post = demap(tt[a], 1 / h2[a], lps[a])
                out["x_soft"][b, t, a], out["nu"][b, t, a] = complex(tt[a]), float(h2[a])
                out["post"][b, t, a] = [float(v) for v in post]
                for i in range(lgM):
                    s0 = [s for s in range(M) if not bits[s, i]]
                    s1 = [s for s in range(M) if bits[s, i]]
                    lav = mp.mpf(float(la[b, t, a, i]))
                    out["llr"][b, t, a, i] = float(mp.log(sum(ez[s] for s in s0))
                                                   - mp.log(sum(ez[s] for s in s1)) - lav)
                    out["llr_maxlog"][b, t, a, i] = float(max(zz[s] for s in s0)
                                                          - max(zz[s] for s in s1) - lav)
                out["moments"][b, t, a] = complex(sum(p * c for p, c in zip(post, cm)))
                out["moments"][b, t, n + a * n + a] = float(sum(p * c for p, c in zip(post, c2)))
            for a in range(n):
                for q in range(n):
                    if a != q:
                        out["moments"][b, t, n + a * n + q] = (out["moments"][b, t, a]
                                                               * np.conj(out["moments"][b, t, q]))
    return out


# ------------------------------------------------------------------ the EM chain
CHAIN_SHAPES = ep.CHAIN_SHAPES
ITERS = eo.ITERS
CHAIN_IA = 0.5


def chain_labels(c):
    return lo.table(c["cons"].size)[1]


@functools.lru_cache(maxsize=None)
def chain_la(shape, vi=0, ia=CHAIN_IA):
    """The a-priori L-values of linear_em_oracle.batch(shape, vi): prior_llr_gaussian at ia on the
    true data bits (ia = 1: every data symbol known)."""
    c = eo.batch(shape, vi)
    rs = np.random.RandomState(9000 + sum(shape))
    la = qam.prior_llr_gaussian(true_bits(c["x_d"], c["cons"], chain_labels(c)), ia, rs)
    la.setflags(write=False)
    return la


def estep(c, b, theta, varn, la, passes=ep.PASSES):
    n_tx = c["n_tx"]
    o = ep_prior_ref(c["y_d"][b:b + 1], c["psi_d"][b:b + 1], c["cons"], theta[None], varn * varn,
                     n_tx, la[b:b + 1], passes=passes, labels=chain_labels(c))
    mom = o["moments"][0]
    return mom[:, :n_tx], mom[:, n_tx:].reshape(-1, n_tx, n_tx), o


def chain(c, b, iters, la, theta0=None, passes=ep.PASSES):
    theta = np.array(c["theta0"][b] if theta0 is None else theta0, dtype=complex)
    thetas, kappa, fail, mr = [], 0.0, False, np.inf
    for _ in range(iters):
        m, S, o = estep(c, b, theta, c["varn"], la, passes)
        kappa, fail = max(kappa, float(o["kappa"].max())), fail or bool(o["fail"].any())
        mr = min(mr, float(o["margin_r"].min()))
        theta = eo.mstep(c, b, m, S)
        thetas.append(theta)
    return dict(thetas=thetas, kappa=kappa, fail=fail, margin_r=mr)


@functools.lru_cache(maxsize=None)
def chain_ref(shape, vi=0, iters=ITERS, ia=CHAIN_IA):
    """ep_oracle.chain_ref with the prior chain_la(shape, vi, ia): per trial the thetas, growth =
    the factor by which a relative 1e-13 perturbation of theta0 grew, and bar = 64 eps kappa
    max(growth, 1), the GPU tier's bound on theta's relative error."""
    c, la = eo.batch(shape, vi), chain_la(shape, vi, ia)
    out = []
    for b in range(eo.B):
        r = chain(c, b, iters, la)
        p = chain(c, b, iters, la, theta0=ep.perturbed(c, b))
        r["growth"] = max(np.linalg.norm(x - y) / np.linalg.norm(x)
                          for x, y in zip(r["thetas"], p["thetas"])) / ep.PERTURB
        r["fail"], r["margin_r"] = r["fail"] or p["fail"], min(r["margin_r"], p["margin_r"])
        r["kappa"] = max(r["kappa"], p["kappa"])
        r["bar"] = 64.0 * EPS * r["kappa"] * max(r["growth"], 1.0)
        out.append(r)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def noise_chain_ref(shape, vi, iters, start, varn_min=1e-6, ia=CHAIN_IA):
    """The restated sbce_em_prior with noise estimation, as ep_oracle.noise_chain_ref."""
    c, la = eo.batch(shape, vi), chain_la(shape, vi, ia)
    out = []
    for b in range(eo.B):
        denom = c["n_rx"] * (c["y_p"].shape[1] + eo.T_D)
        theta, v, status = np.array(c["theta0"][b]), float(start), 0
        hist = np.zeros(iters)
        for l in range(iters):
            m, S, _ = estep(c, b, theta, v, la)
            theta = eo.mstep(c, b, m, S)
            _, Q, _ = no.noise_var_ref(c["y_d"][b], c["y_p"][b], c["u_p"][b], c["psi_d"][b].T, theta,
                                       m, S, parts=True)
            v, flag = no.apply_rules(Q, denom, v, varn_min)
            status |= flag
            hist[l:] = v
        out.append(dict(theta=theta, varn=v, hist=hist, status=status))
    return tuple(out)
