"""Extended-precision restatement of the list (PM / PM-soft), linear-detector (ZF / MMSE) and
Gaussian-prior E-steps of csrc/estep_pm.hip for ANY constellation table, the margin of every
discrete decision they make, and the grid of cases tests/test_gpu_estep_list.py runs.

TEST INFRASTRUCTURE ONLY.  np.longdouble / np.clongdouble throughout, as tests/estep_ref.py.
numpy.linalg takes no extended types: herm_inv is an LDL^H factorisation of its own (the kernels
run a Gauss-Jordan on [G | I]).

The definition restated (header of estep_pm.hip, oracle/pm.py, oracle/detectors.py), per symbol t:
  H_off  = theta[0] + sum_{p < P-1} psi[t][p] theta[p+1]   (the off-by-one channel: builds lists,
           is what ZF / MMSE invert);  H_true = sum_p psi[t][p] theta[p] weighs the list;
  greedy order: repeatedly drop the column with the largest diag((A^H A)^-1), np.argmax = FIRST
           maximum of the real diagonal;
  PM:      A = first NA = int(partition_r / log2 M) + 1 streams of the order, B = the rest,
           z = (B^H B)^-1 B^H (y - A a) for each a in cons^NA (itertools.product order), b = per
           element nearest point (FIRST minimum in table order), x = [a, b] CONCATENATED and then
           used in natural stream order; m = sum w x, S = sum w x x^H with w = 1 (uniform, not
           normalised) or softmax(-||y - H_true x||^2 / varn^2);
  ZF/MMSE: z = (H_off^H H_off [+ varn^2 I])^-1 H_off^H y, s_a = nearest point of z_a, a* = first
           minimum over the streams, flat = a* n_tx (s* = 0) else s* n_tx^2 + a* n_tx + n_tx - 1
           (oracle.detectors.ecul_index), x = row `flat` of the product table; past the table
           (flat >= M^n_tx: the reference raises) the device documents row flat mod M^n_tx;
  Gauss:   A = H_true^H H_true + (varn^2 / varx^2) I, m = A^-1 H_true^H y, C = varn^2 A^-1.
A margin is the relative gap (v2 - v1) / v2 of the two best values of a decision (0 on a tie,
inf where there is no rival).
"""
import numpy as np

import estep_ref as er

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53

MARGIN_MIN = 1e-6        # every decision margin of the grid (planted ties apart)
COND_MAX = 1e6           # cond of every Gram matrix the kernels invert on the grid


def table(name):
    """estep_ref.table plus the two 4-point tables of the empty-B rows."""
    if name == "qam4":
        return np.ascontiguousarray(er.qam(4), dtype=np.complex128)
    if name == "psk4":
        return np.ascontiguousarray(er.psk(4), dtype=np.complex128)
    return er.table(name)


# ------------------------------------------------------------------ margins
def _gap_sorted(v1, v2):
    """(v2 - v1) / v2 for best v1, second v2 (|v2| >= |v1| in magnitude order); 0 on 0 / 0."""
    v1, v2 = np.asarray(v1, dtype=LD), np.asarray(v2, dtype=LD)
    out = np.zeros(v1.shape, dtype=LD)
    np.divide(v2 - v1, v2, out=out, where=v2 != 0)
    return np.abs(out).astype(np.float64)


def gap_min(v, axis=-1):
    """Margin of a first-minimum decision along `axis`: (second - smallest) / second."""
    v = np.asarray(v)
    if v.shape[axis] < 2:
        return np.full(np.delete(v.shape, axis % v.ndim), np.inf)
    s = np.sort(v, axis=axis)
    return _gap_sorted(np.take(s, 0, axis=axis), np.take(s, 1, axis=axis))


def gap_max(v, axis=-1):
    """Margin of a first-maximum decision along `axis`: (largest - second) / largest."""
    v = np.asarray(v)
    if v.shape[axis] < 2:
        return np.full(np.delete(v.shape, axis % v.ndim), np.inf)
    s = np.sort(v, axis=axis)
    n = v.shape[axis]
    return _gap_sorted(np.take(s, n - 2, axis=axis), np.take(s, n - 1, axis=axis))


# ------------------------------------------------------------------ linear algebra
def herm_inv(A):
    """Inverse of Hermitian positive definite A (..., n, n) in extended precision by A = L D L^H
    (L unit lower, D real): A^-1 = L^-H D^-1 L^-1."""
    A = np.asarray(A).astype(CLD)
    n = A.shape[-1]
    L = np.zeros_like(A)
    D = np.zeros(A.shape[:-1], dtype=LD)
    for j in range(n):
        lj = L[..., j, :j]
        D[..., j] = A[..., j, j].real - np.sum((lj.real ** 2 + lj.imag ** 2) * D[..., :j], axis=-1)
        L[..., j, j] = 1
        for i in range(j + 1, n):
            s = np.sum(L[..., i, :j] * np.conj(lj) * D[..., :j], axis=-1)
            L[..., i, j] = (A[..., i, j] - s) / D[..., j]
    X = np.zeros_like(A)                                   # L X = I, row by row
    for i in range(n):
        X[..., i, :] = -np.einsum("...k,...kj->...j", L[..., i, :i], X[..., :i, :])
        X[..., i, i] += 1
    return np.einsum("...ki,...k,...kj->...ij", np.conj(X), LD(1) / D, X)


def _gram(H):
    return np.einsum("...ru,...rv->...uv", np.conj(H), H)


def _cond(G):
    return np.array([np.linalg.cond(g) for g in np.asarray(G).astype(np.complex128)])


def channels(theta, psi_d, n_tx, n_rx):
    """(H_true, H_off), each (T, n_rx, n_tx) extended: H_off weighs theta[p+1] with psi[p]."""
    psi = np.asarray(psi_d)
    off = np.concatenate([np.ones((psi.shape[0], 1), dtype=psi.dtype), psi[:, :-1]], axis=1)
    return er.heff(theta, psi, n_tx, n_rx), er.heff(theta, off, n_tx, n_rx)


def stream_order(H):
    """Greedy order of H (T, n_rx, n_tx): (order (T, n_tx) int, margin (T, n_tx - 1) of each
    step's two largest diagonal entries; the last step has one column and no decision)."""
    T, _, n_tx = H.shape
    cols = np.tile(np.arange(n_tx), (T, 1))
    order = np.zeros((T, n_tx), dtype=int)
    margin = np.full((T, max(n_tx - 1, 0)), np.inf)
    rows = np.arange(T)
    for step in range(n_tx):
        k = n_tx - step
        kmax = np.zeros(T, dtype=int)
        if k > 1:
            Hs = np.take_along_axis(H, cols[:, None, :], axis=2)
            dg = np.einsum("tuu->tu", herm_inv(_gram(Hs))).real
            kmax = np.argmax(dg, axis=1)                   # first maximum
            margin[:, step] = gap_max(dg, axis=1)
        order[:, step] = cols[rows, kmax]
        keep = np.arange(k)[None, :] != kmax[:, None]
        cols = cols[keep].reshape(T, k - 1)
    return order, margin


def _f64(d):
    return {k: (v.astype(np.complex128) if np.iscomplexobj(v) else
                v.astype(np.float64) if v.dtype == LD else v) for k, v in d.items()}


# ------------------------------------------------------------------ PM / PM-soft
def list_moments(theta, y_d, psi_d, cons, varn, n_tx, partition_r):
    """One trial of the list E-step.  Returns m_u, S_u (uniform weights), m_s, S_s (posterior
    weights), order (T, n_tx), lst (T, JA, n_tx) table indices of the candidates, the margins
    g_order (T, n_tx - 1), g_near (T, JA, nB), cond (T,) of H_off^H H_off, and what the bounds
    need: ax (T, n_tx) = sum_j |x_j|, axx (T, n_tx, n_tx) = sum_j |x_a||x_b|, kap_num (T,) =
    max_j sum_r (|y_r| + sum_a |H_true[r][a]||x_a|)^2."""
    cons = np.asarray(cons, dtype=np.complex128)
    c = cons.astype(CLD)
    M = cons.size
    y = np.asarray(y_d).astype(CLD)
    T, n_rx = y.shape
    Ht, Ho = channels(theta, psi_d, n_tx, n_rx)
    order, g_order = stream_order(Ho)
    NA = int(partition_r / np.log2(M)) + 1
    nB, JA = n_tx - NA, M ** NA
    ia = er._hyp(cons, NA, 0, JA)                           # (JA, NA), first stream slowest
    A = np.take_along_axis(Ho, order[:, None, :NA], axis=2)                   # (T, n_rx, NA)
    lst = np.zeros((T, JA, n_tx), dtype=int)
    lst[:, :, :NA] = ia[None]
    g_near = np.full((T, JA, nB), np.inf)
    if nB:
        Bm = np.take_along_axis(Ho, order[:, None, NA:], axis=2)              # (T, n_rx, nB)
        GB = np.einsum("tuv,trv->tur", herm_inv(_gram(Bm)), np.conj(Bm))      # (T, nB, n_rx)
        res = y[:, None, :] - np.einsum("tra,ja->tjr", A, c[ia])              # (T, JA, n_rx)
        z = np.einsum("tur,tjr->tju", GB, res)
        dz = z[..., None] - c
        d = dz.real ** 2 + dz.imag ** 2                                       # (T, JA, nB, M)
        lst[:, :, NA:] = np.argmin(d, axis=-1)              # first minimum in table order
        g_near = gap_min(d, axis=-1)
    x = c[lst]                                              # (T, JA, n_tx): natural order from here
    out = dict(order=order, lst=lst, g_order=g_order, g_near=g_near, cond=_cond(_gram(Ho)))
    out["m_u"] = x.sum(axis=1)
    out["S_u"] = np.einsum("tja,tjb->tab", x, np.conj(x))
    r = y[:, None, :] - np.einsum("tra,tja->tjr", Ht, x)
    dist = np.sum(r.real ** 2 + r.imag ** 2, axis=2)        # (T, JA)
    w = np.exp(-(dist - dist.min(axis=1, keepdims=True)) / (LD(varn) * LD(varn)))
    w /= w.sum(axis=1, keepdims=True)
    out["m_s"] = np.einsum("tj,tja->ta", w, x)
    out["S_s"] = np.einsum("tj,tja,tjb->tab", w, x, np.conj(x))
    ab = np.abs(x)
    out["ax"] = ab.sum(axis=1)
    out["axx"] = np.einsum("tja,tjb->tab", ab, ab)
    up = np.abs(y)[:, None, :] + np.einsum("tra,tja->tjr", np.abs(Ht), ab)
    out["kap_num"] = np.max(np.sum(up ** 2, axis=2), axis=1)
    return _f64(out)


# ------------------------------------------------------------------ ZF / MMSE
def flat_index(a, s, n_tx):
    """oracle.detectors.ecul_index's flat argmin from the winning stream a and table index s."""
    return a * n_tx if s == 0 else s * n_tx * n_tx + a * n_tx + n_tx - 1


def det_moments(theta, y_d, psi_d, cons, varn, n_tx, kind):
    """One trial of the ZF / MMSE hard decision.  Returns flat (T,) python ints as object array,
    over (T,) bool = flat >= M^n_tx, m (T, n_tx), S, and the margins g_near (T, n_tx), g_stream
    (T,), cond (T,) of the inverted Gram matrix."""
    cons = np.asarray(cons, dtype=np.complex128)
    c = cons.astype(CLD)
    M = cons.size
    y = np.asarray(y_d).astype(CLD)
    T, n_rx = y.shape
    _, Ho = channels(theta, psi_d, n_tx, n_rx)
    G = _gram(Ho)
    if kind == "mmse":
        G = G + (LD(varn) * LD(varn)) * np.eye(n_tx, dtype=LD)
    z = np.einsum("tuv,trv,tr->tu", herm_inv(G), np.conj(Ho), y)
    dz = z[..., None] - c
    d = dz.real ** 2 + dz.imag ** 2                         # (T, n_tx, M)
    sb = np.argmin(d, axis=2)
    db = d.min(axis=2)
    a_star = np.argmin(db, axis=1)
    J = M ** n_tx
    flat = np.array([flat_index(int(a), int(sb[t, a]), n_tx) for t, a in enumerate(a_star)],
                    dtype=object)
    row = np.array([f % J for f in flat], dtype=object)
    idx = np.array([[(int(f) // M ** (n_tx - 1 - q)) % M for q in range(n_tx)] for f in row])
    m = cons[idx]
    return dict(flat=flat, over=np.array([f >= J for f in flat]), m=m,
                S=m[:, :, None] * np.conj(m[:, None, :]), idx=idx,
                g_near=gap_min(d, axis=2), g_stream=gap_min(db, axis=1), cond=_cond(G))


# ------------------------------------------------------------------ Gauss
def gauss_moments(theta, y_d, psi, varn, varx, n_tx):
    """One trial of the Gaussian-prior E-step (psi (T, N) WITHOUT a direct-path column, theta the
    reduced channel of N n_tx n_rx entries): m (T, n_tx), C (T, n_tx, n_tx), cond (T,) of A."""
    y = np.asarray(y_d).astype(CLD)
    T, n_rx = y.shape
    H = er.heff(theta, psi, n_tx, n_rx)
    s2, vx = LD(varn) * LD(varn), LD(varx) * LD(varx)
    A = _gram(H) + (s2 / vx) * np.eye(n_tx, dtype=LD)
    Ai = herm_inv(A)
    m = np.einsum("tuv,trv,tr->tu", Ai, np.conj(H), y)
    return _f64(dict(m=m, C=s2 * Ai, cond=_cond(A)))


def gauss_float64(theta, y_d, psi, varn, varx, n_tx):
    """numpy's own float64 evaluation of the same formula (np.linalg.inv): its distance from
    gauss_moments sets the constant of the Gauss bar."""
    y = np.asarray(y_d, dtype=np.complex128)
    T, n_rx = y.shape
    th = np.asarray(theta, dtype=np.complex128).reshape(np.shape(psi)[1], n_tx, n_rx)
    H = np.einsum("tp,par->tra", np.asarray(psi, dtype=np.complex128), th)
    Ai = np.linalg.inv(np.conj(np.swapaxes(H, 1, 2)) @ H + (varn ** 2 / varx ** 2) * np.eye(n_tx))
    m = np.einsum("tuv,trv,tr->tu", Ai, np.conj(H), y)
    return m, varn ** 2 * Ai


# Gauss bar: |err| <= GAUSS_C cond(A) 2^-53 relative to max|m| and max|C|.  GAUSS_C is 4 x the
# largest ratio err / (cond(A) 2^-53 max|.|) of gauss_float64 against gauss_moments over the row 7
# grid (measured 9.28, at cond(A) ~ 1 where the n_tx- and P-term sums dominate;
# tests/test_pm_ref.py::test_gauss_constant repeats the measurement).
GAUSS_C = 38.0


# ------------------------------------------------------------------ the dispatch, restated
def route(mode, n_tx, n_rx, M, partition_r, arm, nsym):
    """launch_estep_pm restated: the kernel instantiation a call reaches, as a string.  arm: ''
    (default), 't', 'q' or 'wave' (SBCE_PM_IMPL)."""
    w = arm == "wave"
    code = {"pm": 2, "pm_soft": 3, "zf": 4, "mmse": 5, "gauss": 6}[mode]
    if mode in ("zf", "mmse") and n_tx <= 2 and not w:
        return f"det_thread<{n_tx},{n_rx},{code}>"
    if mode in ("pm", "pm_soft"):
        NA = int(partition_r / np.log2(M)) + 1
        if n_tx == 2 and NA == 1 and not w:
            quad = arm == "q" or (arm != "t" and nsym < 96 * 1024)
            return f"pm_{'quad' if quad else 'thread'}<{code},{n_rx}>"
    return f"pm_wave<{code}>"


def reachable():
    """Every instantiation launch_estep_pm can reach with n_rx >= n_tx (MMSE: any n_rx)."""
    out = {f"pm_wave<{c}>" for c in (2, 3, 4, 5, 6)}
    for nt in (1, 2):
        for nr in range(1, 9):
            if nr >= nt:
                out.add(f"det_thread<{nt},{nr},4>")
            out.add(f"det_thread<{nt},{nr},5>")
    for nr in range(2, 9):
        for c in (2, 3):
            out |= {f"pm_quad<{c},{nr}>", f"pm_thread<{c},{nr}>"}
    return out


# ------------------------------------------------------------------ the grid
B = 3
_CYCLE = ("qam64", "qam64_perm", "qam16_uneven", "cross32", "apsk64", "bpsk")
_DET, _PM, _ALL4 = ("zf", "mmse"), ("pm", "pm_soft"), ("", "t", "q", "wave")


def _case(row, n_tx, n_rx, N, tab, snr, modes, arms=("",), r=0, varx=1.0):
    return dict(row=row, n_tx=n_tx, n_rx=n_rx, N=N, tab=tab, snr=snr, modes=tuple(modes),
                arms=tuple(arms), r=r, varx=varx, T_d=23 if n_tx <= 2 else 6)


def _grid():
    g = []
    for n_rx in range(1, 9):                                                   # row 1
        for tab in ("qam16_perm", "psk8"):
            g.append(_case(1, 1, n_rx, 2, tab, 10, _DET, ("", "wave")))
    for shift, snr in ((0, -5), (3, 25)):                                      # row 2
        for n_rx in range(1, 9):
            tab = _CYCLE[(n_rx - 1 + shift) % 6]
            g.append(_case(2, 2, n_rx, 3, tab, snr, _DET if n_rx >= 2 else ("mmse",),
                           ("", "wave")))
    for shift, snr in ((0, -5), (2, 10), (4, 33)):                             # row 3
        for n_rx in range(2, 9):
            tab = _CYCLE[(n_rx - 2 + shift) % 6]
            g.append(_case(3, 2, n_rx, 3, tab, snr, _PM, _ALL4, r=0 if tab == "bpsk" else 1))
    g += [_case(4, 1, 1, 2, "qam16", 10, _PM), _case(4, 1, 5, 2, "psk8", 10, _PM),      # row 4
          _case(4, 2, 2, 3, "qam4", 10, _PM, r=2), _case(4, 2, 2, 3, "psk4", 10, _PM, r=2),
          _case(4, 2, 6, 3, "qam4", 10, _PM, r=2), _case(4, 2, 6, 3, "psk4", 10, _PM, r=2),
          _case(4, 3, 4, 1, "bpsk", 10, _PM, r=2)]
    g += [_case(5, 3, 3, 2, "psk8", 10, _PM, r=3), _case(5, 4, 4, 2, "qam4", 10, _PM, r=4),  # row 5
          _case(5, 4, 6, 2, "psk16", 10, _PM, r=1), _case(5, 5, 6, 1, "bpsk", 10, _PM, r=3),
          _case(5, 6, 7, 1, "qam16", 10, _PM), _case(5, 7, 8, 1, "qam64_perm", 10, _PM),
          _case(5, 8, 8, 2, "qam16", 0, _PM, r=1), _case(5, 8, 8, 2, "qam16", 20, _PM, r=1),
          _case(5, 3, 5, 0, "qam16_uneven", 10, _PM, r=1)]
    g += [_case(6, 3, 3, 2, "bpsk", 10, _DET), _case(6, 4, 6, 2, "cross32", 10, _DET),   # row 6
          _case(6, 8, 8, 2, "qam16", 10, _DET), _case(6, 5, 7, 0, "qam16_perm", 10, _DET),
          _case(6, 3, 1, 2, "qam16", 10, ("mmse",)), _case(6, 8, 1, 1, "qam16", 10, ("mmse",)),
          _case(6, 5, 3, 1, "qam16", 10, ("mmse",))]
    for n_tx, n_rx in ((2, 2), (8, 8), (8, 1), (1, 8), (5, 3)):                # row 7
        for varx in (1.0, 0.5):
            for snr in (0, 20):
                c = _case(7, n_tx, n_rx, 3, "qam16", snr, ("gauss",), varx=varx)
                c["T_d"] = 6
                g.append(c)
    for i, c in enumerate(g):
        c["pos"] = i
        c["seed"] = RESEED.get(i, i)
        c["id"] = (f"r{c['row']}-{c['n_tx']}x{c['n_rx']}-N{c['N']}-{c['tab']}-{c['snr']}dB"
                   f"-r{c['r']}" + (f"-vx{c['varx']}" if c["row"] == 7 else ""))
    return g


# The seed of a case is its position in the grid; where that draw misses a condition the next
# free seed (counting on from the grid's size) is taken and recorded here: {position: seed}.
RESEED = {}

GRID = _grid()
VARN_SCALE = (0.5, 1.0, 2.0)            # the per-trial noise cases: x the nominal varn


def by_row(row):
    return [c for c in GRID if c["row"] == row]


def pick(row, **match):
    """The first case of `row` whose fields equal `match`."""
    return next(c for c in by_row(row) if all(c[k] == v for k, v in match.items()))


# per-trial noise: one case each of rows 2, 3, 5, 6, in MMSE and PM-soft
VARN_CASES = [pick(2, n_rx=5, tab="qam64_perm"), pick(3, n_rx=7, tab="qam64_perm"),
              pick(5, n_tx=8, snr=20), pick(6, n_tx=8, n_rx=8)]
# independence of the trials: one case per row, tiled to B = 300
INDEP_CASES = [pick(1, n_rx=3, tab="qam16_perm"), pick(2, n_rx=2), pick(3, n_rx=5, snr=-5),
               pick(4, n_tx=2, n_rx=2, tab="qam4"), pick(5, tab="psk16"), pick(6, tab="cross32"),
               pick(7, n_tx=5, snr=20, varx=0.5)]


def _tie_cases():
    """Planted exact ties (ZF / MMSE): integer grids, n_tx = 1, 2 (thread and wave arms) and one
    n_tx = 3 (the wave kernel alone).  Their seeds go on from the grid's."""
    out = []
    for tab in ("qam16", "qam16_perm", "qam64_perm"):
        out += [_case(0, 1, 3, 2, tab, 10, _DET, ("", "wave")),
                _case(0, 2, 3, 2, tab, 10, _DET, ("", "wave"))]
    out.append(_case(0, 3, 4, 2, "qam16_perm", 10, _DET))
    for k, c in enumerate(out):
        c["pos"] = c["seed"] = len(GRID) + k
        c["id"] = f"tie-{c['n_tx']}x{c['n_rx']}-{c['tab']}"
    return out


TIE_CASES = _tie_cases()


def tie_inputs(case):
    """(y_d with every second symbol zeroed, the (T_d,) mask of the zeroed symbols): z is then
    exactly 0 there, the four innermost grid points tie exactly, and so do the streams."""
    y = batch(case)["y_d"].copy()
    mask = np.arange(y.shape[1]) % 2 == 1
    y[:, mask] = 0
    return y, mask


def varn_vector(case):
    return np.array(VARN_SCALE) * batch(case)["varn"]


def covered():
    """The instantiations the grid's calls reach (route over every case, mode and arm)."""
    out = set()
    for c in GRID:
        nsym = B * c["T_d"]
        M = table(c["tab"]).size
        for mode in c["modes"]:
            for arm in c["arms"]:
                out.add(route(mode, c["n_tx"], c["n_rx"], M, c["r"], arm, nsym))
    return out


def batch(case):
    """The case's inputs (estep_ref.synthetic_batch), cached."""
    key = ("batch", case["pos"])
    if key not in _cache:
        _cache[key] = er.synthetic_batch(table(case["tab"]), B, case["n_tx"], case["n_rx"],
                                         case["N"], case["T_d"], case["snr"], case["seed"])
    return _cache[key]


def gauss_inputs(case, kind):
    """Row 7: psi without the direct-path column and the matching part of theta."""
    b = batch(case)
    k0 = case["n_tx"] * case["n_rx"]
    return b["theta_" + kind][:, k0:], b["psi_d"][:, :, 1:]


_cache = {}


def _stack(per):
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def reference(case, kind, mode, varn=None, y_d=None):
    """The restatement of `case` for theta_`kind` and `mode` ('pm' / 'pm_soft' share one entry,
    so do the arms), stacked over the B trials and cached.  varn: a (B,) vector of per-trial
    values (default: the batch's).  y_d: other data symbols (the planted ties), not cached."""
    fam = "pm" if mode in _PM else mode
    vkey = None if varn is None else tuple(np.asarray(varn, dtype=float).tolist())
    key = ("ref", case["pos"], kind, fam, vkey)
    if y_d is None and key in _cache:
        return _cache[key]
    b = batch(case)
    v = np.full(B, b["varn"]) if varn is None else np.asarray(varn, dtype=float)
    y = b["y_d"] if y_d is None else y_d
    n_tx, cons = case["n_tx"], b["cons"]
    per = []
    for i in range(B):
        if fam == "pm":
            per.append(list_moments(b["theta_" + kind][i], y[i], b["psi_d"][i], cons, v[i], n_tx,
                                    case["r"]))
        elif fam == "gauss":
            th, psi = gauss_inputs(case, kind)
            per.append(gauss_moments(th[i], y[i], psi[i], v[i], case["varx"], n_tx))
        else:
            per.append(det_moments(b["theta_" + kind][i], y[i], b["psi_d"][i], cons, v[i], n_tx,
                                   fam))
    out = _stack(per)
    if y_d is None:
        _cache[key] = out
    return out


def check_conditions(case, varn=None, y_d=None, exempt=None):
    """The grid's own conditions for one case, every theta and mode: no symbol is left out, every
    decision margin >= MARGIN_MIN and every inverted Gram matrix has cond <= COND_MAX.  exempt: a
    (T_d,) mask of planted-tie symbols, whose margins must be exactly 0 instead.  Raises
    AssertionError naming the smallest margin / largest cond otherwise."""
    for kind in ("narrow", "wide"):
        for fam in sorted({"pm" if m in _PM else m for m in case["modes"]}):
            ref = reference(case, kind, fam, varn, y_d)
            tag = (case["id"], kind, fam)
            assert ref["cond"].max() <= COND_MAX, (tag, "cond", ref["cond"].max())
            for g in ("g_order", "g_near", "g_stream"):
                if g not in ref or not ref[g].size:
                    continue
                v = ref[g]
                if exempt is not None and g != "g_order":
                    tie = v[:, exempt]
                    assert np.all(tie[np.isfinite(tie)] == 0), (tag, g, "planted tie", tie.max())
                    v = v[:, ~exempt]
                assert v.min() >= MARGIN_MIN, (tag, g, v.min())
