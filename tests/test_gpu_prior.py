"""GPU tier of soft-input expectation propagation (csrc/ep_prior.h, csrc/estep_linear.hip and
the prior kernel of csrc/detect_linear.hip; sbce_detect_linear_prior, sbce_estep_prior,
sbce_em_prior): every output against the NumPy restatement (tests/prior_oracle.py), the prior-free
calls bit for bit, tiling and determinism, the degenerate symbols, the EM chain against the
restated loop, both ends of the a-priori information, the error codes and graph capture.

Bounds: integer outputs exact outside the symbols whose relative MAP-decision gap is below 1e-6
(the CPU tier, tests/test_prior.py, asserts there are at most 1 % of them and that no other branch
can flip on rounding); each continuous output within 16 max(r_k, 1) eps kappa_t scale, r_k
measured on the CPU against a 50-digit copy of the restatement (prior_oracle.C_BY_OUTPUT); the
chain's theta within 64 eps kappa_b max(growth_b, 1) per trial, both factors from the oracle's own
run of that trial.  Nothing comes from the kernel."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

from conftest import rel
import ep_oracle as ep
import linear_em_oracle as eo
import linear_oracle as lo
import prior_oracle as po
import solve_ref as sr

pytestmark = pytest.mark.gpu

ALL = ("x_soft", "nu", "x_hat", "idx", "llr", "post", "moments", "status")
KEYS = ALL + ("err",)
CONT = {"x_soft", "nu", "post", "llr", "llr_maxlog", "moments"}
EINVAL, EUNSUPPORTED = -1, -2
STATUS_BAD = 1 | 4 | 16 | 32


def _moments(m, S):
    return np.concatenate([m, S.reshape(*m.shape[:2], -1)], axis=2)


def _estep(sbce, c, varn, la, passes=None):
    m, S, st = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], mode="ep",
                                return_status=True, ep_passes=passes, prior_llr=la,
                                labels=c["labels"])
    return _moments(m, S), st


def _detect(sbce, c, varn, la, passes=None, **kw):
    kw.setdefault("labels", c["labels"])
    kw.setdefault("want", ALL)
    return sbce.detect_linear_prior_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"],
                                          la, kind="ep" if passes is None else ("ep", passes), **kw)


def _args(c, sl=slice(None)):
    return c["y_d"][sl], c["y_p"][sl], c["psi_d"][sl], c["u_p"][sl], c["cons"]


def _sub(c, sl):
    return {k: (v[sl] if k in ("y", "psi", "theta", "x", "la") else v) for k, v in c.items()}


def _check_parity(sbce, c, varn, o, la, passes, what, ok=None):
    r = _detect(sbce, c, varn, la, passes, x_d_true=c["x"])
    rm = _detect(sbce, c, varn, la, passes, maxlog=True, want=("llr",))
    mom, st = _estep(sbce, c, varn, la, passes)
    rat = po.ratios(dict(r, llr_maxlog=rm["llr"]), o, c["cons"], ok=ok)
    rat_e = po.ratios({"moments": mom}, o, c["cons"], ok=ok)["moments"]
    guarded = o["gap"] < po.GAP
    print(f"{what} p {passes}: max kappa {o['kappa'][~o['fail']].max():.3g}, guarded "
          f"{int(guarded.sum())}, err / (eps kappa scale): estep moments {rat_e:.3g}, "
          + ", ".join(f"{k} {v:.3g}" for k, v in rat.items())
          + " (bounds " + ", ".join(f"{k} {v:.3g}" for k, v in po.C_BY_OUTPUT.items()) + ")")
    for k in ("x_soft", "x_hat", "post", "llr", "moments"):
        assert np.all(np.isfinite(r[k])), k
    assert np.all(np.isfinite(mom)) and np.all(np.isfinite(rm["llr"]))
    keep = ~guarded
    assert r["idx"].dtype == np.int32
    assert np.array_equal(r["idx"][keep], o["idx"][keep])
    assert np.array_equal(r["x_hat"][keep], o["x_hat"][keep])
    if not guarded.any():
        assert np.array_equal(r["err"], o["err"])
    assert np.array_equal(r["status"], o["status"])                     # SBCE_STATUS_NONHPD
    assert np.array_equal(st, 4 * o["status"])                          # SBCE_STATUS_DETECTOR
    assert set(rat) == CONT
    assert rat_e <= po.C_BY_OUTPUT["moments"], rat_e
    for k, v in rat.items():
        assert v <= po.C_BY_OUTPUT[k], (k, v)
    return r, rm, mom


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("passes", po.PASSES)
@pytest.mark.parametrize("si,vi,ii", po.CASES)
def test_parity_with_restatement(sbce, si, vi, ii, passes):
    """Every sbce_detect_linear_prior output (exact and max-log L-values; the noise given per trial
    through sigma2_t) and sbce_estep_prior's moments; +inf, -inf, NaN and 1e3 planted in la."""
    c, varn, o = po.case(si, vi, ii), po.VARNS[vi], po.ref(si, vi, ii, passes)
    _check_parity(sbce, c, np.full(po.B, varn), o, c["la"], passes,
                  f"shape {po.SHAPES[si]} varn {varn} I_A {po.IAS[ii]}")


def test_zero_prior_is_close_to_the_prior_free_kernels(sbce):
    """la = 0 on a zero-mean table is the prior-free EP in exact arithmetic: the two kernels agree
    within the parity bound (not bitwise: the prior kernel forms its start from the table)."""
    si, vi = 3, 0
    c, varn, o = ep.case(si, vi), ep.VARNS[vi], ep.ref(si, vi)
    la = np.zeros(c["x"].shape + (4,))
    r = _detect(sbce, c, varn, la)
    r0 = _detect(sbce, c, varn, None)
    sc = lo.scales(o, c["cons"])
    for k in ("x_soft", "nu", "post", "llr", "moments"):
        assert np.max(np.abs(r[k] - r0[k]) / sc[k]) <= ep.C_BY_OUTPUT[k], k
    assert np.array_equal(r["idx"], r0["idx"])


# ------------------------------------------------------------------ 2. no prior
def _raw_detect(sbce, c, sigma2, passes, la, fill, maxlog=False, entry="prior", sl=slice(None)):
    """sbce_detect_linear_prior (or sbce_detect_linear) through the raw binding into outputs
    pre-filled with `fill`; la: a device tensor or None (NULL)."""
    import torch
    L = sbce._lib
    lib = L.load()
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k][sl] if k != "cons" else c[k])).cuda()
           for k in ("y", "psi", "cons", "theta", "x")}
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    Bn, T_d, n_rx = dev["y"].shape
    P, M, n_tx = dev["psi"].shape[2], dev["cons"].shape[0], c["n_tx"]
    lgM = max(int(M - 1).bit_length(), 1)
    c128, f64, i32 = torch.complex128, torch.float64, torch.int32
    shapes = {"x_soft": ((Bn, T_d, n_tx), c128), "nu": ((Bn, T_d, n_tx), f64),
              "x_hat": ((Bn, T_d, n_tx), c128), "idx": ((Bn, T_d, n_tx), i32),
              "post": ((Bn, T_d, n_tx, M), f64), "llr": ((Bn, T_d, n_tx, lgM), f64),
              "moments": ((Bn, T_d, n_tx + n_tx * n_tx), c128), "status": ((Bn,), i32),
              "err": ((Bn, 2), i32)}
    out = {k: torch.full(s, fill, dtype=t, device="cuda") for k, (s, t) in shapes.items()}
    dims = L.LinearDims(Bn, n_tx, n_rx, P, T_d, M, L.SBCE_LINEAR_EP,
                        L.linear_ep_passes(passes) | (L.SBCE_DETECT_MAXLOG if maxlog else 0),
                        float(sigma2), lo.default_es(c["cons"]))
    ptrs = L.LinearPtrs(y_d=dev["y"].data_ptr(), psi_d=dev["psi"].data_ptr(),
                        cons=dev["cons"].data_ptr(), theta=dev["theta"].data_ptr(),
                        labels=lab.data_ptr(), x_d_true=dev["x"].data_ptr(),
                        x_soft=out["x_soft"].data_ptr(), nu=out["nu"].data_ptr(),
                        x_hat=out["x_hat"].data_ptr(), idx_hat=out["idx"].data_ptr(),
                        post=out["post"].data_ptr(), llr=out["llr"].data_ptr(),
                        err=out["err"].data_ptr(), moments=out["moments"].data_ptr(),
                        status=out["status"].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "prior":
        rc = lib.sbce_detect_linear_prior(dims, ptrs, la.data_ptr() if la is not None else None,
                                          stream)
    else:
        rc = lib.sbce_detect_linear(dims, ptrs, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_null_prior_is_the_existing_detector(sbce):
    c = ep.case(5, 1)
    a = _raw_detect(sbce, c, 1.0, 5, None, 3, entry="plain")
    b = _raw_detect(sbce, c, 1.0, 5, None, 9, entry="prior")
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def _em_raw(sbce, c, iters, pr, nz=False, cv=False, mode=None, over=None, want_iters_done=True):
    """sbce_em_prior through the raw binding on a fresh staging: dict(rc, theta, status, varn)."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    st = em._Staged(torch, *_args(c), c["theta0"], c["varn"], solve=L.SBCE_SOLVE_CHOL,
                    check="theta0", clone=True)
    keep = []
    nzo = cvo = None
    est = None
    if nz:
        nzo, est, hist, scr = em._noise_opts(torch, lib, st, 1e-6, iters)
        keep += [hist, scr]
    if cv:
        dth = torch.zeros((st.B, iters), dtype=torch.float64, device="cuda")
        scr = em._scratch(torch, lib.sbce_conv_workspace_bytes, "sbce_conv_workspace_bytes",
                          ctypes.byref(st.dims), 0)
        cvo = L.ConvOpts(0.0, 0.0, iters, 0, dth.data_ptr(), None, scr.data_ptr(), scr.numel())
        keep += [dth, scr]
    ptrs = st.ptrs(**(over or {}))
    if not want_iters_done:
        ptrs.iters_done = None
    rc = lib.sbce_em_prior(st.dims, ptrs, iters, L.SBCE_ESTEP_EP if mode is None else mode,
                           L.SBCE_SOLVE_CHOL, ctypes.byref(pr) if pr is not None else None,
                           ctypes.byref(nzo) if nzo is not None else None,
                           ctypes.byref(cvo) if cvo is not None else None,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(rc=rc, theta=st.theta.cpu().numpy(), status=st.status.cpu().numpy(),
                varn=None if est is None else est.cpu().numpy(), st=st)


def test_null_prior_is_the_existing_estep_and_chains(sbce):
    """pr == NULL and pr->la == NULL through sbce_estep_prior and sbce_em_prior (plain, with nz,
    with cv) at (5, 6, 3, 20), 4 iterations: the bits of sbce_estep, sbce_em, sbce_em_noise and
    sbce_em_conv."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    c = eo.batch(eo.S56, 0)
    n_tx = c["n_tx"]
    m, S = sbce.estep_batch(c["y_d"], c["psi_d"], c["cons"], c["theta0"], c["varn"], n_tx, mode="ep")
    st = em._Staged(torch, *_args(c), c["theta0"], c["varn"], workspace=False)
    for pr in (None, L.PriorOpts(None, None, 0)):
        mom = torch.full((eo.B, eo.T_D, n_tx + n_tx * n_tx), -7.0, dtype=torch.complex128,
                         device="cuda")
        rc = lib.sbce_estep_prior(st.dims, st.ptrs(), L.SBCE_ESTEP_EP,
                                  ctypes.byref(pr) if pr is not None else None, mom.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(mom.cpu().numpy(), _moments(m, S))
        a = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep")
        r = _em_raw(sbce, c, eo.ITERS, pr)
        assert r["rc"] == 0 and np.array_equal(r["theta"], a["theta"])
        assert np.array_equal(r["status"], a["status"])
        a = sbce.em_batch_noise(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep")
        r = _em_raw(sbce, c, eo.ITERS, pr, nz=True)
        assert r["rc"] == 0 and np.array_equal(r["theta"], a["theta"])
        assert np.array_equal(r["varn"], a["varn"])
        a = sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], tol_theta=0.0,
                               min_iters=eo.ITERS, mode="ep")
        r = _em_raw(sbce, c, eo.ITERS, pr, cv=True)
        assert r["rc"] == 0 and np.array_equal(r["theta"], a["theta"])


# ------------------------------------------------------------------ 3. tiling and determinism
def test_several_workgroups_determinism_and_degenerate_symbols(sbce):
    """T_d = 70: three workgroups per trial, the last ragged; priors |La| <= 4.  Trial 1
    (varn = 1e-8, equal channel columns from symbol 40 on) loses a pivot on exactly the planted
    symbols: post = the a-priori pmf, llr = 0, moments from it, x_soft = 0, nu = +inf, the trial
    flagged from its second and third workgroup; the other trials untouched.  B = 3 is bitwise
    three B = 1 calls, and two runs into differently pre-filled outputs agree bit for bit."""
    import torch
    c, varn = dict(lo.chunk_case()), np.array(ep.CHUNK_VARN_T)
    c["la"] = po.chunk_la()
    o = po.chunk_ref()
    n_tx, n_rx, P, T_d, M = lo.CHUNK_SHAPE
    bad = o["fail"]
    assert np.abs(c["la"]).max() <= 4.0
    r, rm, mom = _check_parity(sbce, c, varn, o, c["la"], None, "T_d 70", ok=~bad)
    assert bad.sum() == T_d - lo.DEFECT_T0 and not bad[[0, 2]].any() and list(r["status"]) == [0, 1, 0]
    assert np.all(r["x_soft"][bad] == 0) and np.all(r["nu"][bad] == np.inf)
    assert np.all(r["llr"][bad] == 0) and np.all(rm["llr"][bad] == 0)
    tiny = 64 * lo.EPS
    assert np.abs(r["post"][bad] - o["prior"][bad]).max() <= tiny
    assert np.abs(r["post"][bad] - 1.0 / M).max() > 1e-3       # no longer the uniform pmf
    scale = np.abs(c["cons"]).max() ** 2
    for got in (mom, r["moments"]):
        assert np.abs(got[bad] - o["moments"][bad]).max() <= M * tiny * scale
    assert np.array_equal(r["idx"][bad], np.argmax(o["prior"][bad], axis=-1))
    la_d = torch.from_numpy(np.ascontiguousarray(c["la"])).cuda()
    for b in range(3):
        one = _detect(sbce, _sub(c, slice(b, b + 1)), float(varn[b]), c["la"][b:b + 1],
                      x_d_true=c["x"][b:b + 1])
        for k in KEYS:
            assert np.array_equal(r[k][b:b + 1], one[k]), (k, b)
        assert np.array_equal(_estep(sbce, _sub(c, slice(b, b + 1)), float(varn[b]),
                                     c["la"][b:b + 1])[0], mom[b:b + 1])
    x = _raw_detect(sbce, c, lo.CHUNK_VARN ** 2, 5, la_d, 1)
    y = _raw_detect(sbce, c, lo.CHUNK_VARN ** 2, 5, la_d, 77)
    for k in KEYS:
        assert np.array_equal(x[k], y[k]), k


# ------------------------------------------------------------------ 4. the chain
@pytest.mark.parametrize("shape", po.CHAIN_SHAPES, ids=eo.chain_id)
def test_chain_parity_with_restated_loop(sbce, shape):
    """sbce_em_prior, 4 iterations at I_A = 0.5, on the four M-step routes; with cv (theta rule,
    min_iters = iters) theta is bitwise the plain prior chain's, and so is the first iteration of
    the noise-estimating chain (its first E-step runs at the caller's parameter)."""
    c, la = eo.batch(shape, 0), po.chain_la(shape)
    lab = po.chain_labels(c)
    r = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep", prior_llr=la, labels=lab)
    ref = po.chain_ref(shape)
    errs = [rel(r["theta"][b], ref[b]["thetas"][-1]) for b in range(eo.B)]
    bars = [ref[b]["bar"] for b in range(eo.B)]
    print(f"{shape} prior chain: theta rel err per trial " + " ".join(f"{e:.2e}" for e in errs)
          + "; bars " + " ".join(f"{v:.2e}" for v in bars) + f", status {r['status']}")
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert not (r["status"] & STATUS_BAD).any()
    for e, bar in zip(errs, bars):
        assert e <= bar
    cv = sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], tol_theta=0.0,
                            min_iters=eo.ITERS, mode="ep", prior_llr=la, labels=lab)
    assert np.array_equal(cv["theta"], r["theta"])
    one = sbce.em_batch(*_args(c), c["varn"], 1, c["theta0"], mode="ep", prior_llr=la, labels=lab)
    nz1 = sbce.em_batch_noise(*_args(c), c["varn"], 1, c["theta0"], mode="ep", prior_llr=la,
                              labels=lab)
    assert np.array_equal(nz1["theta"], one["theta"])


def test_em_noise_matches_restated_loop(sbce):
    shape = eo.S56
    c, la = eo.batch(shape, 0), po.chain_la(shape)
    r = sbce.em_batch_noise(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep", prior_llr=la,
                            labels=po.chain_labels(c))
    ref = po.noise_chain_ref(shape, 0, eo.ITERS, c["varn"])
    e_th = max(rel(r["theta"][b], ref[b]["theta"]) for b in range(eo.B))
    e_h = np.abs(r["hist"] / np.stack([q["hist"] for q in ref]) - 1).max()
    bar = max(q["bar"] for q in po.chain_ref(shape))
    print(f"em_noise {shape} prior: theta {e_th:.3e} hist {e_h:.3e} bar {bar:.3e}")
    assert not r["status"].any() and not any(q["status"] for q in ref)
    assert e_th <= bar and e_h <= bar


# ------------------------------------------------------------------ 5. both ends
@pytest.mark.parametrize("shape", [eo.S56, eo.S88], ids=eo.chain_id)
def test_known_symbols_give_the_genie_mstep_and_its_bound(sbce, shape):
    """prior_llr_known(x_d): one iteration gives the theta of mstep_batch at genie_moments(x_d)
    within the solve bar max(1e-12, 1e-15 cond(R)) of tests/solve_ref.py (the moments differ from
    the genie's by <= M e^-64), and its NMSE, averaged over the batch, lies within 4 standard
    deviations of crb_batch(kind="genie")'s mean: theta_hat - theta ~ CN(0, sigma2 R^-1) per
    receive row, so ||.||^2 has variance n_rx sigma2^2 tr(R^-2) (computed here from R)."""
    c = eo.batch(shape, 0)
    lab = po.chain_labels(c)
    n_tx, n_rx = c["n_tx"], c["n_rx"]
    la = sbce.qam.prior_llr_known(c["x_d"], c["cons"], lab)
    assert np.all(np.isinf(la))
    r = sbce.em_batch(*_args(c), c["varn"], 1, c["theta0"], mode="ep", prior_llr=la, labels=lab)
    m, S = sbce.genie_moments(c["x_d"])
    th, R, rhs, st = sbce.mstep_batch(*_args(c), m, S, c["varn"])
    s2 = c["varn"] ** 2
    crb = sbce.crb_batch(c["y_d"], c["y_p"], c["psi_d"], c["u_p"], c["cons"], n_tx, s2, kind="genie",
                         x_d_true=c["x_d"], h_true=c["h"], want=("bound",))
    nm, var = [], []
    for b in range(eo.B):
        Rb = sr.herm_lower(R[b], np.complex128)
        bar = sr.forward_bar(float(np.linalg.cond(Rb)))
        e = rel(r["theta"][b], th[b])
        print(f"{shape} trial {b}: theta vs genie M-step {e:.2e} (bar {bar:.2e})")
        assert e <= bar
        hn = np.linalg.norm(c["h"][b]) ** 2
        nm.append(np.linalg.norm(r["theta"][b] - c["h"][b]) ** 2 / hn)
        Ri = np.linalg.inv(Rb)
        var.append(n_rx * s2 * s2 * np.real(np.trace(Ri @ Ri)) / hn ** 2)
    spread = np.sqrt(np.sum(var)) / eo.B
    print(f"{shape}: mean NMSE {np.mean(nm):.4e}, genie bound {crb['bound'].mean():.4e}, "
          f"sampling spread of the mean {spread:.2e}")
    assert abs(np.mean(nm) - crb["bound"].mean()) <= 4.0 * spread


# ------------------------------------------------------------------ 6. arguments
def test_error_codes_before_any_launch(sbce):
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    c = eo.batch(eo.S34, 0)
    n_tx = c["n_tx"]
    lab_np = po.chain_labels(c)
    la = torch.from_numpy(np.ascontiguousarray(po.chain_la(eo.S34))).cuda()
    lab = torch.from_numpy(lab_np).cuda()
    st = em._Staged(torch, *_args(c), c["theta0"], c["varn"], solve=L.SBCE_SOLVE_CHOL,
                    check="theta0", clone=True)
    before = st.theta.cpu().numpy().copy()
    mom = torch.full((eo.B, eo.T_D, n_tx + n_tx * n_tx), -7.0, dtype=torch.complex128, device="cuda")
    xbuf = torch.zeros((eo.B, eo.T_D, n_tx), dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    EP = L.SBCE_ESTEP_EP

    def em_rc(pr, mode=EP, cv=None, **ptr):
        return lib.sbce_em_prior(st.dims, st.ptrs(**ptr), 2, mode, L.SBCE_SOLVE_CHOL,
                                 ctypes.byref(pr), None, cv, stream)

    def estep_rc(pr, mode=EP, **ptr):
        return lib.sbce_estep_prior(st.dims, st.ptrs(**ptr), mode, ctypes.byref(pr), mom.data_ptr(),
                                    stream)

    good = L.PriorOpts(la.data_ptr(), lab.data_ptr(), 0)
    for rc in (em_rc, estep_rc):
        assert rc(L.PriorOpts(la.data_ptr(), None, 0)) == EINVAL              # la without labels
        assert rc(L.PriorOpts(la.data_ptr() + 4, lab.data_ptr(), 0)) == EINVAL
        assert rc(L.PriorOpts(la.data_ptr(), lab.data_ptr() + 2, 0)) == EINVAL
        assert rc(L.PriorOpts(la.data_ptr(), lab.data_ptr(), 1)) == EINVAL
        assert rc(L.PriorOpts(None, None, 1)) == EINVAL
        assert rc(good, x_sup=xbuf) == EINVAL
        assert rc(good, mode=L.SBCE_ESTEP_MMSE_SOFT) == EUNSUPPORTED
        assert rc(good, mode=L.SBCE_ESTEP_SOFT) == EUNSUPPORTED
    dth = torch.zeros((eo.B, 2), dtype=torch.float64, device="cuda")
    llh = torch.zeros((eo.B, 2), dtype=torch.float64, device="cuda")
    scr = em._scratch(torch, lib.sbce_conv_workspace_bytes, "sbce_conv_workspace_bytes",
                      ctypes.byref(st.dims), 1)
    cv = L.ConvOpts(0.0, 0.0, 2, 0, dth.data_ptr(), llh.data_ptr(), scr.data_ptr(), scr.numel())
    assert em_rc(good, cv=ctypes.byref(cv)) == EUNSUPPORTED                   # ll_hist with a prior
    # the detector
    d = ep.case(1, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    dlab = torch.from_numpy(np.ascontiguousarray(d["labels"], dtype=np.int32)).cuda()
    dla = torch.zeros((3, 5, 2, 4), dtype=torch.float64, device="cuda")
    out = torch.full((3, 5, 2), -7.0, dtype=torch.float64, device="cuda")

    def det(la_ptr, labels=True, **over):
        v = dict(batch=3, n_tx=2, n_rx=2, n_psi=3, t_d=5, m=16, kind=L.SBCE_LINEAR_EP, flags=0,
                 sigma2=0.09, es=10.0)
        v.update(over)
        dd = L.LinearDims(*[v[f] for f, _ in L.LinearDims._fields_])
        p = L.LinearPtrs(y_d=dev[0].data_ptr(), psi_d=dev[1].data_ptr(), cons=dev[2].data_ptr(),
                         theta=dev[3].data_ptr(), nu=out.data_ptr(),
                         labels=dlab.data_ptr() if labels else None)
        return lib.sbce_detect_linear_prior(dd, p, la_ptr, stream)

    assert det(dla.data_ptr(), labels=False) == EINVAL
    assert det(dla.data_ptr() + 4) == EINVAL
    assert det(dla.data_ptr(), kind=L.SBCE_LINEAR_MMSE) == EUNSUPPORTED
    assert det(dla.data_ptr(), kind=L.SBCE_LINEAR_ZF) == EUNSUPPORTED
    assert det(dla.data_ptr(), n_tx=9, n_rx=8) == EUNSUPPORTED
    assert det(dla.data_ptr(), sigma2=0.0) == EINVAL and det(dla.data_ptr(), kind=2) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(st.theta.cpu().numpy(), before)          # nothing was launched
    assert np.all(mom.cpu().numpy() == -7.0) and np.all(out.cpu().numpy() == -7.0)
    assert det(dla.data_ptr()) == 0 and estep_rc(good) == 0 and em_rc(good) == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() > 0) and not np.any(mom.cpu().numpy() == -7.0)
    assert not np.array_equal(st.theta.cpu().numpy(), before)
    with pytest.raises(ValueError):
        sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="mmse_soft",
                      prior_llr=po.chain_la(eo.S34))
    with pytest.raises(ValueError):
        sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep",
                      prior_llr=po.chain_la(eo.S34)[:, :, :, :2])


# ------------------------------------------------------------------ 7. graph capture
def test_graph_capture_replays_the_eager_bits(sbce):
    """One sbce_detect_linear_prior call and one 2-iteration engine chain, each captured on one
    stream and replayed twice into refilled outputs: the eager bits."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    c = po.case(4, 0, 1)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(c["x"])).cuda()
    la = torch.from_numpy(np.ascontiguousarray(c["la"])).cuda()
    args = (torch, *dev, c["n_tx"], "ep", 0.09, None, lo.default_es(c["cons"]), lab, xd, False, ALL, 5)
    eager = {k: v.cpu().numpy() for k, v in em._detect_linear_call(*args, la=la).items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = em._detect_linear_call(*args, la=la)
    for _ in range(2):
        for v in out.values():
            v.fill_(1)
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert np.array_equal(out[k].cpu().numpy(), v), k
    o = po.ref(4, 0, 1, 5)
    assert np.array_equal(eager["idx"], o["idx"]) and np.array_equal(eager["err"], o["err"])

    b = eo.batch(eo.S56, 0)
    batch = dict(y_d=b["y_d"], y_p=b["y_p"], psi_d=b["psi_d"], u_p=b["u_p"], cons=b["cons"],
                 theta0=b["theta0"])
    cla, clab = po.chain_la(eo.S56), po.chain_labels(b)
    want = sbce.em_batch(*_args(b), b["varn"], 2, b["theta0"], mode="ep", prior_llr=cla,
                         labels=clab)["theta"]
    eng = sbce.EMEngine(batch, b["varn"], mode="ep", prior_llr=cla, labels=clab)
    assert np.array_equal(eng.run(2).cpu().numpy(), want)
    torch.cuda.synchronize()
    g2 = eng.capture(2)
    for _ in range(2):
        eng.theta.fill_(0)
        g2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(eng.theta.cpu().numpy(), want)
    d = eng.detect_linear(kind="ep", want=("x_soft", "llr"))
    d2 = sbce.detect_linear_prior_batch(b["y_d"], b["psi_d"], b["cons"], want, b["varn"], b["n_tx"],
                                        cla, labels=clab, want=("x_soft", "llr"))
    for k in ("x_soft", "llr"):
        assert np.array_equal(d[k], d2[k]), k


def _captured_node_types(stream, fn):
    """Capture what fn() enqueues on `stream` (raw HIP stream capture through the runtime torch
    loaded; every buffer is allocated before) and return (node types, instantiate-and-launch)."""
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    hip.hipGraphDestroy.argtypes = [vp]
    assert hip.hipStreamBeginCapture(stream, 1) == 0        # hipStreamCaptureModeThreadLocal
    try:
        rc = fn()
    finally:
        graph = vp()
        end = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
    assert rc == 0 and end == 0 and graph.value
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (vp * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for nd in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(nd, ctypes.byref(t)) == 0
        types.append(t.value)
    assert hip.hipGraphDestroy(graph) == 0
    return types


def test_captured_graphs_hold_kernel_nodes_only(sbce):
    """One sbce_detect_linear_prior call (err and status set: the zeroing kernel and the prior
    kernel) and one 2-iteration sbce_em_prior chain (iters_done left out: its fill is the chain's
    only memset), captured on one stream: every node is a kernel node (hipGraphNodeTypeKernel = 0),
    and the chain has as many nodes as the prior-free sbce_em."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    c = po.case(3, 0, 0)
    n_tx, n_rx, P, T_d, M = po.SHAPES[3]
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta", "x")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    la = torch.from_numpy(np.ascontiguousarray(c["la"])).cuda()
    llr = torch.zeros((po.B, T_d, n_tx, 4), dtype=torch.float64, device="cuda")
    err = torch.zeros((po.B, 2), dtype=torch.int32, device="cuda")
    status = torch.zeros(po.B, dtype=torch.int32, device="cuda")
    dims = L.LinearDims(po.B, n_tx, n_rx, P, T_d, M, L.SBCE_LINEAR_EP, 0, 0.09, lo.default_es(c["cons"]))
    ptrs = L.LinearPtrs(y_d=dev[0].data_ptr(), psi_d=dev[1].data_ptr(), cons=dev[2].data_ptr(),
                        theta=dev[3].data_ptr(), labels=lab.data_ptr(), x_d_true=dev[4].data_ptr(),
                        llr=llr.data_ptr(), err=err.data_ptr(), status=status.data_ptr())
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    types = _captured_node_types(s.cuda_stream, lambda: lib.sbce_detect_linear_prior(
        dims, ptrs, la.data_ptr(), s.cuda_stream))
    print(f"detector graph node types {types}")
    assert types == [0, 0]

    b = eo.batch(eo.S56, 0)
    st = em._Staged(torch, *_args(b), b["theta0"], b["varn"], solve=L.SBCE_SOLVE_CHOL,
                    check="theta0", clone=True)
    cla = torch.from_numpy(np.ascontiguousarray(po.chain_la(eo.S56))).cuda()
    clab = torch.from_numpy(po.chain_labels(b)).cuda()
    pr = L.PriorOpts(cla.data_ptr(), clab.data_ptr(), 0)
    pp = st.ptrs()
    pp.iters_done = None
    torch.cuda.synchronize()
    with_prior = _captured_node_types(s.cuda_stream, lambda: lib.sbce_em_prior(
        st.dims, pp, 2, L.SBCE_ESTEP_EP, L.SBCE_SOLVE_CHOL, ctypes.byref(pr), None, None,
        s.cuda_stream))
    without = _captured_node_types(s.cuda_stream, lambda: lib.sbce_em(
        st.dims, pp, 2, L.SBCE_ESTEP_EP, L.SBCE_SOLVE_CHOL, s.cuda_stream))
    print(f"chain graph node types {with_prior}")
    assert with_prior and set(with_prior) == {0} and len(with_prior) == len(without)
    torch.cuda.synchronize()
