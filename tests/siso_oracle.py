"""Plain NumPy restatement of the soft-in / soft-out decoder (include/sbce.h sbce_siso_decode):
the dense log-domain forward-backward recursion over every (state, input) pair, written from the
header's definition with no normalisation and no schedule.  Beside it an independent brute-force
a-posteriori computation over all 2^n_info codewords (n_info <= 10), a 50-digit (mpmath) copy that
fixes the bounds' constants, the seeded parity cases, and the code-aided (turbo) loop on
prior_oracle's EM chain and detector.  Test infrastructure only: the product has no CPU path."""
import functools
import importlib
import itertools

import numpy as np

from conftest import PKG

qam = importlib.import_module(PKG + ".qam")
codec = importlib.import_module(PKG + ".codec")

EPS = np.finfo(float).eps
CLAMP = 64.0              # |L| after the load (csrc/ep_prior.h kPriorClamp)
GAP = 1e-6                # as prior_oracle.GAP: |lapp_u| below GAP x scale is a guarded bit

# (K, generators in octal) of the parity cases
CODES = ((3, (0o7, 0o5)), (4, (0o15, 0o17)), (5, (0o23, 0o35)), (6, (0o53, 0o75)),
         (7, (0o133, 0o171)), (7, (0o133, 0o171, 0o165)))
B_MAX = 17
# (la_u, perm, maxlog): each switch is met on and off
VARIANTS = ((False, False, False), (True, True, False), (True, False, True), (False, True, True))
IA_C, IA_U = 0.5, 0.3     # mutual information of the consistent-Gaussian L-values of a case

# The bounds' constants, by prior_oracle's method: r_k = the largest ratio of |float64 restatement
# - 50-digit restatement| to scales() -- eps x the largest finite |A_t| entering the output's two
# log-sums, at least eps x 1 for the log of the class sum itself -- over the first codeword of
# every parity case (every code, n_info, termination and variant); C_k = 16 max(r_k, 1), 16 being
# the margin prior_oracle gives a different summation order.  Measured by measure_constants()
# (tests/test_siso.py checks a subset against them); nothing here comes from the kernel.
# Measured r_k: lapp_u 4.07 and le_c 3.55 ((7; 133, 171, 165), n_info 200, unterminated, plain
# variant), lapp_u_maxlog 3.75 ((6; 53, 75), n_info 200, unterminated), le_c_maxlog 3.78 ((7; 133,
# 171, 165), n_info 200, terminated): the restatement keeps the metrics unnormalised, so its
# rounding grows with the length of the recursion as |A|, the unit, does.
R_BY_OUTPUT = dict(lapp_u=4.1, le_c=3.6, lapp_u_maxlog=3.8, le_c_maxlog=3.8)
C_BY_OUTPUT = {k: 16.0 * max(r, 1.0) for k, r in R_BY_OUTPUT.items()}


# (expected code, (batch, n_info, K, n, generators, flags)): dims sbce_siso_decode refuses before
# any HIP call (flags 2 = SBCE_SISO_TERMINATED)
BAD_DIMS = ((-2, (2, 5, 8, 2, (0o133, 0o171, 0), 2)),      # K out of range
            (-2, (2, 5, 2, 2, (3, 3, 0), 2)),
            (-2, (2, 5, 3, 4, (7, 5, 0), 2)),              # n out of range
            (-2, (2, 5, 3, 1, (7, 5, 0), 2)),
            (-1, (2, 5, 3, 2, (6, 5, 0), 2)),              # bit 0 not set
            (-1, (2, 5, 3, 2, (7, 3, 0), 2)),              # bit K-1 not set
            (-1, (2, 5, 3, 2, (15, 5, 0), 2)),             # a bit above K-1
            (-1, (2, 5, 3, 3, (7, 5, 0), 2)),              # n = 3 with the third generator missing
            (-1, (2, 5, 3, 2, (7, 5, 0), 4)),              # unknown flag
            (-1, (0, 5, 3, 2, (7, 5, 0), 2)),
            (-1, (2, 0, 3, 2, (7, 5, 0), 2)),
            (-2, (1, 16383, 3, 2, (7, 5, 0), 2)),          # n_steps = 16385
            (-2, (1, 16385, 3, 2, (7, 5, 0), 0)))


def sanitise(l):
    l = np.array(l, dtype=float)
    l[np.isnan(l)] = 0.0
    return np.clip(l, -CLAMP, CLAMP)


def n_info_list(K):
    return sorted({1, 2, K - 1, 33, 200})


def batches(K):
    return sorted({1, B_MAX, (64 >> (K - 1)) + 1})


def code_of(ci, terminated):
    K, gens = CODES[ci]
    return codec.ConvCode(gens, K, terminated)


def branch_tables(code):
    """nxt[s][u] and cbits[s][u][j] of the header's trellis."""
    S, K = code.n_states, code.K
    nxt = np.zeros((S, 2), dtype=int)
    cb = np.zeros((S, 2, code.n), dtype=int)
    for s in range(S):
        for u in range(2):
            w = (u << (K - 1)) | s
            nxt[s, u] = w >> 1
            for j, g in enumerate(code.generators):
                cb[s, u, j] = bin(w & g).count("1") & 1
    return nxt, cb


def _lse(x, axis, maxlog):
    """Max-shifted log-sum-exp along ``axis``; -inf for nothing but -inf."""
    m = np.max(x, axis=axis)
    if maxlog:
        return m
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.sum(np.exp(x - np.expand_dims(ms, axis)),
                                                           axis=axis)), -np.inf)


def siso_ref(lc, code, la_u=None, perm=None, maxlog=False):
    """The definition, densely: lc (B, n_steps n) -> dict(lapp_u, u_hat, le_c (B, n_steps n) at the
    caller's positions, scale (B, n_steps): the largest finite |A_t|, at least 1)."""
    lc = np.asarray(lc, dtype=float)
    B, nc = lc.shape
    n, S = code.n, code.n_states
    n_info = code.n_info_for(nc)
    T = code.n_steps(n_info)
    perm = np.arange(nc) if perm is None else np.asarray(perm)
    L = sanitise(lc)[:, perm].reshape(B, T, n)
    La = np.zeros((B, T))
    if la_u is not None:
        La[:, :n_info] = sanitise(la_u)
    nxt, cb = branch_tables(code)
    # gamma[b, t, s, u]
    gam = -np.einsum("suj,btj->btsu", cb.astype(float), L)
    gam[..., 1] -= La[:, :, None]
    if code.terminated:
        gam[:, n_info:, :, 1] = -np.inf
    alpha = np.full((B, T + 1, S), -np.inf)
    alpha[:, 0, 0] = 0.0
    for t in range(T):
        into = np.full((B, S, 2), -np.inf)             # the two branches into each s'
        cnt = np.zeros(S, dtype=int)
        for s in range(S):
            for u in range(2):
                into[:, nxt[s, u], cnt[nxt[s, u]]] = alpha[:, t, s] + gam[:, t, s, u]
                cnt[nxt[s, u]] += 1
        alpha[:, t + 1] = _lse(into, 2, maxlog)
    beta = np.full((B, T + 1, S), -np.inf)
    if code.terminated:
        beta[:, T, 0] = 0.0
    else:
        beta[:, T] = 0.0
    for t in range(T - 1, -1, -1):
        beta[:, t] = _lse(gam[:, t] + beta[:, t + 1][:, nxt], 2, maxlog)
    A = alpha[:, :T, :, None] + gam + beta[:, 1:][:, :, nxt]          # (B, T, S, 2)
    flat = A.reshape(B, T, 2 * S)
    ub = np.tile(np.array([0, 1]), S)
    cbf = cb.reshape(2 * S, n)

    def split(mask):                                   # lse over class 0 minus lse over class 1
        with np.errstate(invalid="ignore"):
            l0 = _lse(np.where(mask == 0, flat, -np.inf), 2, maxlog)
            l1 = _lse(np.where(mask == 1, flat, -np.inf), 2, maxlog)
            return l0 - l1
    lapp = split(ub)[:, :n_info]
    le = np.stack([split(cbf[:, j]) for j in range(n)], axis=2) - L
    le_c = np.empty((B, nc))
    le_c[:, perm] = le.reshape(B, nc)
    fin = np.where(np.isfinite(flat), np.abs(flat), 0.0)
    scale = np.maximum(fin.max(axis=2), 1.0)
    return dict(lapp_u=lapp, u_hat=(lapp < 0).astype(np.int32), le_c=le_c, scale=scale)


def scales(o, code, perm=None):
    """Error units of (lapp_u, le_c): EPS x the step's scale, le_c at the caller's positions."""
    B, T = o["scale"].shape
    n_info = o["lapp_u"].shape[1]
    su = EPS * o["scale"][:, :n_info]
    sc = np.repeat(EPS * o["scale"], code.n, axis=1)
    out = np.empty_like(sc)
    out[:, np.arange(T * code.n) if perm is None else np.asarray(perm)] = sc
    return dict(lapp_u=su, le_c=out)


def guarded(o):
    """Bits whose decision is not compared: |lapp_u| below GAP x the step's scale."""
    return np.abs(o["lapp_u"]) < GAP * o["scale"][:, :o["lapp_u"].shape[1]]


def empty_classes(code, n_info):
    """(n_steps, n) int: +1 where the class c_j = 1 of the step is structurally empty (le_c = +inf),
    -1 where c_j = 0 is, else 0 -- from reachability alone."""
    nxt, cb = branch_tables(code)
    S, T = code.n_states, code.n_steps(n_info)
    fw = np.zeros((T + 1, S), dtype=bool)
    fw[0, 0] = True
    for t in range(T):
        for s in np.nonzero(fw[t])[0]:
            for u in range(1 if (code.terminated and t >= n_info) else 2):
                fw[t + 1, nxt[s, u]] = True
    bw = np.zeros((T + 1, S), dtype=bool)
    if code.terminated:
        bw[T, 0] = True
    else:
        bw[T] = True
    for t in range(T - 1, -1, -1):
        for s in range(S):
            for u in range(1 if (code.terminated and t >= n_info) else 2):
                bw[t, s] |= bw[t + 1, nxt[s, u]]
    out = np.zeros((T, code.n), dtype=int)
    for t in range(T):
        seen = np.zeros((code.n, 2), dtype=bool)
        for s in range(S):
            for u in range(1 if (code.terminated and t >= n_info) else 2):
                if fw[t, s] and bw[t + 1, nxt[s, u]]:
                    for j in range(code.n):
                        seen[j, cb[s, u, j]] = True
        for j in range(code.n):
            out[t, j] = 0 if seen[j].all() else (1 if seen[j, 0] else -1)
    return out


def brute_force(lc, code, la_u=None, perm=None):
    """A-posteriori L-values by enumeration of all 2^n_info codewords (one codeword's lc (nc,)):
    no trellis, only the encoder."""
    lc = sanitise(np.asarray(lc, dtype=float))
    nc = lc.size
    n_info = code.n_info_for(nc)
    assert n_info <= 10
    perm = np.arange(nc) if perm is None else np.asarray(perm)
    U = np.array(list(itertools.product((0, 1), repeat=n_info)), dtype=int)
    C = code.encode(U).astype(float)                   # (2^n_info, nc) in the decoder's order
    L = lc[perm]
    lp = -C @ L
    if la_u is not None:
        lp = lp - U @ sanitise(la_u)

    def split(bit):
        with np.errstate(invalid="ignore"):
            l0 = _lse(np.where(bit == 0, lp, -np.inf), 0, False)
            l1 = _lse(np.where(bit == 1, lp, -np.inf), 0, False)
            return l0 - l1
    lapp = np.array([split(U[:, t]) for t in range(n_info)])
    le = np.array([split(C[:, k]) for k in range(nc)]) - L
    le_c = np.empty(nc)
    le_c[perm] = le
    return dict(lapp_u=lapp, le_c=le_c)


def siso_ref_mp(lc, code, la_u=None, perm=None, maxlog=False, digits=50):
    """siso_ref for ONE codeword in ``digits``-digit arithmetic (mpmath): (lapp_u, le_c) as lists of
    mpf, le_c at the caller's positions."""
    import mpmath as mp
    mp.mp.dps = digits
    ninf = mp.mpf("-inf")
    lc = sanitise(np.asarray(lc, dtype=float))
    nc = lc.size
    n, S = code.n, code.n_states
    n_info = code.n_info_for(nc)
    T = code.n_steps(n_info)
    perm = np.arange(nc) if perm is None else np.asarray(perm)
    L = [[mp.mpf(float(lc[perm[t * n + j]])) for j in range(n)] for t in range(T)]
    La = [mp.mpf(0)] * T
    if la_u is not None:
        lau = sanitise(la_u)
        La = [mp.mpf(float(lau[t])) if t < n_info else mp.mpf(0) for t in range(T)]
    nxt, cb = branch_tables(code)

    def lse(xs):
        xs = [x for x in xs if x != ninf]
        if not xs:
            return ninf
        m = max(xs)
        return m if maxlog else m + mp.log(mp.fsum(mp.exp(x - m) for x in xs))

    def gamma(t, s, u):
        if u and code.terminated and t >= n_info:
            return ninf
        return -mp.fsum(L[t][j] for j in range(n) if cb[s, u, j]) - (La[t] if u else 0)
    alpha = [[ninf] * S for _ in range(T + 1)]
    alpha[0][0] = mp.mpf(0)
    for t in range(T):
        into = [[] for _ in range(S)]
        for s in range(S):
            if alpha[t][s] == ninf:
                continue
            for u in range(2):
                g = gamma(t, s, u)
                if g != ninf:
                    into[nxt[s, u]].append(alpha[t][s] + g)
        alpha[t + 1] = [lse(v) for v in into]
    beta = [[ninf] * S for _ in range(T + 1)]
    beta[T] = [mp.mpf(0) if (s == 0 or not code.terminated) else ninf for s in range(S)]
    for t in range(T - 1, -1, -1):
        for s in range(S):
            beta[t][s] = lse([gamma(t, s, u) + beta[t + 1][nxt[s, u]] for u in range(2)
                              if gamma(t, s, u) != ninf and beta[t + 1][nxt[s, u]] != ninf])
    lapp, le = [], [None] * nc
    for t in range(T):
        A = {}
        for s in range(S):
            for u in range(2):
                g, b = gamma(t, s, u), beta[t + 1][nxt[s, u]]
                A[s, u] = ninf if (alpha[t][s] == ninf or g == ninf or b == ninf) \
                    else alpha[t][s] + g + b

        def split(cls):
            l0 = lse([A[k] for k in A if cls(*k) == 0])
            l1 = lse([A[k] for k in A if cls(*k) == 1])
            if l0 == ninf:
                return ninf
            return mp.mpf("inf") if l1 == ninf else l0 - l1
        if t < n_info:
            lapp.append(split(lambda s, u: u))
        for j in range(n):
            le[perm[t * n + j]] = split(lambda s, u, j=j: cb[s, u, j]) - L[t][j]
    return lapp, le


# ------------------------------------------------------------------ the seeded parity cases
@functools.lru_cache(maxsize=None)
def case(ci, n_info, terminated):
    """The B_MAX codewords of one (code, n_info, termination): u, lc on the interleaved positions,
    la_u and the interleaver.  A call at B < B_MAX takes the first B codewords."""
    code = code_of(ci, terminated)
    seed = 7000 + 1000 * ci + 2 * n_info + int(terminated)
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (B_MAX, n_info))
    c = code.encode(u)
    nc = c.shape[1]
    perm = codec.random_interleaver(nc, seed)
    sent = np.empty_like(c)
    sent[:, perm] = c                                  # coded bit k travels at position perm[k]
    lc = qam.prior_llr_gaussian(sent, IA_C, rng)
    la_u = qam.prior_llr_gaussian(u, IA_U, rng)
    for a in (u, lc, la_u, perm):
        a.setflags(write=False)
    return dict(code=code, u=u, lc=lc, la_u=la_u, perm=perm)


def case_inputs(ci, n_info, terminated, variant):
    """(lc, la_u or None, perm or None, maxlog) of a variant.  Without the interleaver the same
    lc values are simply read in the natural order: another, equally valid, noisy codeword."""
    c = case(ci, n_info, terminated)
    use_la, use_perm, maxlog = variant
    return c["lc"], (c["la_u"] if use_la else None), (c["perm"] if use_perm else None), maxlog


@functools.lru_cache(maxsize=None)
def case_ref(ci, n_info, terminated, variant):
    c = case(ci, n_info, terminated)
    lc, la, perm, maxlog = case_inputs(ci, n_info, terminated, variant)
    o = siso_ref(lc, c["code"], la, perm, maxlog)
    for v in o.values():
        v.setflags(write=False)
    return o


def all_cases():
    return [(ci, ni, term, v) for ci in range(len(CODES)) for ni in n_info_list(CODES[ci][0])
            for term in (True, False) for v in VARIANTS]


def ratios_mp(ci, n_info, terminated, variant):
    """r of the first codeword of a case: max |float64 - 50-digit| / scales(), per output."""
    c = case(ci, n_info, terminated)
    lc, la, perm, maxlog = case_inputs(ci, n_info, terminated, variant)
    o = siso_ref(lc[:1], c["code"], None if la is None else la[:1], perm, maxlog)
    sc = scales(o, c["code"], perm)
    lapp, le = siso_ref_mp(lc[0], c["code"], None if la is None else la[0], perm, maxlog)
    r = {}
    for k, mpv in (("lapp_u", lapp), ("le_c", le)):
        worst = 0.0
        for got, want, s in zip(o[k][0], mpv, sc[k][0]):
            if np.isinf(got):
                assert float(want) == got, (k, got, want)
                continue
            worst = max(worst, float(abs(want - float(got))) / s)
        r[k] = worst
    return r


def measure_constants(cases=None):
    """The r_k behind R_BY_OUTPUT (minutes at the full list)."""
    worst = {}
    for cs in (all_cases() if cases is None else cases):
        for k, v in ratios_mp(*cs).items():
            key = k + ("_maxlog" if cs[3][2] else "")
            if v > worst.get(key, (0.0, None))[0]:
                worst[key] = (v, cs)
    return worst


# ------------------------------------------------------------------ the code-aided (turbo) loop
# Seed, SNR and pilot length chosen on the CPU (T_p = 16 = L leaves the pilot least squares square
# and ill-conditioned: NMSE_0 > 1 and no iteration recovers; at T_p = 20 and 10 dB the restated loop
# gives 198 -> 153 -> 136 bit errors of 1520 and NMSE 0.072 -> 0.058 -> 0.052, genie bound 0.014)
TURBO = dict(n_tx=4, n_rx=4, N=3, M=16, T_p=20, T_d=24, B=8, snr_db=10.0, seed=11, outer=3, itera=3,
             passes=5)


@functools.lru_cache(maxsize=None)
def turbo_case():
    """The coded batch of the loop tests: B codewords of the (7, 5) terminated code, interleaved,
    Gray-mapped to 16-QAM on 4 streams x T_d = 24 symbols (384 coded bits, 190 information bits)."""
    t = TURBO
    code = codec.ConvCode((0o7, 0o5), 3, True)
    lgM = 4
    nc = t["T_d"] * t["n_tx"] * lgM
    n_info = code.n_info_for(nc)
    rng = np.random.default_rng(t["seed"])
    u = rng.integers(0, 2, (t["B"], n_info))
    c = code.encode(u)
    perm = codec.random_interleaver(nc, t["seed"])
    sent = np.empty_like(c)
    sent[:, perm] = c
    cons = qam.qam_constellation(t["M"])
    labels = qam.gray_labeling(t["M"])
    x_d = qam.map_bits(sent.reshape(t["B"], t["T_d"], t["n_tx"], lgM), cons, labels)
    # the channel model of linear_em_oracle.batch (signal_model's DFT pilots never excite the last
    # RIS element, so its pilot estimate is a quarter of the channel short at any SNR): theta ~
    # CN(0, 1/P), random unit-modulus phases, Kronecker pilots, theta0 = the pilot least squares;
    # varn is the noise variance the data carry, snr_db = es / varn per stream and antenna
    B, n_tx, n_rx, P, T_p, T_d = t["B"], t["n_tx"], t["n_rx"], t["N"] + 1, t["T_p"], t["T_d"]
    varn = float(np.mean(np.abs(cons) ** 2)) * 10.0 ** (-t["snr_db"] / 10.0)
    K = P * n_tx * n_rx
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)
    h = cn(B, K) / np.sqrt(P)
    psi_d = np.exp(2j * np.pi * rng.random((B, T_d, P)))
    psi_p = np.exp(2j * np.pi * rng.random((B, T_p, P)))
    x_p = cons[rng.integers(0, t["M"], (B, T_p, n_tx))]
    u_p = (psi_p[:, :, :, None] * x_p[:, :, None, :]).reshape(B, T_p, P * n_tx)
    H = np.einsum("btp,bpar->btra", psi_d, h.reshape(B, P, n_tx, n_rx))
    y_d = np.einsum("btra,bta->btr", H, x_d) + np.sqrt(varn) * cn(B, T_d, n_rx)
    y_p = np.einsum("btl,blr->btr", u_p, h.reshape(B, P * n_tx, n_rx)) + np.sqrt(varn) * cn(B, T_p, n_rx)
    theta0 = np.stack([np.linalg.lstsq(u_p[b], y_p[b], rcond=None)[0].reshape(-1) for b in range(B)])
    d = dict(y_d=y_d, y_p=y_p, psi_d=psi_d, u_p=u_p, cons=cons, theta0=theta0, h=h, x_d=x_d,
             n_tx=n_tx, n_rx=n_rx, varn=varn, code=code, perm=perm, u=u, labels=labels, sent=sent)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def turbo_ref(d, outer, itera, passes):
    """The loop of em.turbo_em_batch on the CPU: per outer iteration the EM chain and the detector
    of prior_oracle with the decoder's extrinsic L-values as the prior, then siso_ref.  Returns the
    list of per-iteration dicts (theta, llr, la, lapp_u, u_hat, scale, la_in)."""
    import prior_oracle as po
    B, T_d, n_tx = d["x_d"].shape
    lgM = 4
    sig = float(np.sqrt(d["varn"]))                    # exit_chart.py's convention: the EM gets sqrt
    c = dict(d, varn=sig)
    theta = d["theta0"].copy()
    la = np.zeros((B, T_d, n_tx, lgM))
    out = []
    for _ in range(outer):
        th = np.stack([po.chain(c, b, itera, la, theta0=theta[b], passes=passes)["thetas"][-1]
                       for b in range(B)]).reshape(B, -1)
        det = po.ep_prior_ref(d["y_d"], d["psi_d"], d["cons"], th, d["varn"], n_tx, la,
                              passes=passes, labels=d["labels"])
        llr = det["llr"].reshape(B, -1)
        o = siso_ref(llr, d["code"], None, d["perm"])
        out.append(dict(theta=th, llr=llr, la_in=la, la=o["le_c"].reshape(B, T_d, n_tx, lgM),
                        lapp_u=o["lapp_u"], u_hat=o["u_hat"], scale=o["scale"], sigma=sig))
        theta, la = th, out[-1]["la"]
    return out
