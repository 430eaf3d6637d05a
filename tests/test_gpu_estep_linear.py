"""GPU tier of the soft ZF / MMSE E-steps (csrc/estep_linear.hip; SBCE_ESTEP_MMSE_SOFT,
SBCE_ESTEP_ZF_SOFT): the E-step against the NumPy restatement and against sbce_detect_linear, the
EM chain through sbce_em / sbce_em_noise / sbce_em_conv / sbce_em_multi against the restated loop
(tests/linear_em_oracle.py), batch independence, per-trial variances, the `done` skip, graph
capture and the error codes.

Bounds: the E-step's moments within C eps kappa_t scale, the bound tests/linear_oracle.py derives
for this arithmetic (C = 282.4 from a 50-digit copy of the restatement); the chain at the relative
1e-9 of the project's chain tests, on batches whose conditioning tests/test_linear_em.py guards."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

from conftest import rel
import linear_em_oracle as eo
import linear_oracle as lo

pytestmark = pytest.mark.gpu


def _moments(m, S):
    return np.concatenate([m, S.reshape(*m.shape[:2], -1)], axis=2)


def _estep(sbce, c, varn, kind):
    m, S, st = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"],
                                mode=kind + "_soft", return_status=True)
    return _moments(m, S), st


def _args(c, sl=slice(None)):
    return c["y_d"][sl], c["y_p"][sl], c["psi_d"][sl], c["u_p"][sl], c["cons"]


# ------------------------------------------------------------------ 1. E-step parity
@pytest.mark.parametrize("si,vi,kind", lo.CASES)
def test_estep_parity_with_restatement(sbce, si, vi, kind):
    c, varn, o = lo.case(si, vi), lo.VARNS[vi], lo.ref(si, vi, kind)
    mom, st = _estep(sbce, c, varn, kind)
    rat = lo.ratios({"moments": mom}, o, c["cons"])["moments"]
    print(f"shape {lo.SHAPES[si]} varn {varn} {kind}_soft: max kappa {o['kappa'].max():.3g}, "
          f"moments err / (eps kappa scale) {rat:.3g} (bound {lo.C})")
    assert np.all(np.isfinite(mom)) and not st.any()
    assert rat <= lo.C


@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_estep_several_workgroups_per_trial(sbce, kind):
    """T_d = 70: three workgroups per trial, the last ragged.  ZF: trial 1 has a singular A from
    symbol 40 on -- those symbols carry the uniform posterior's moments exactly (16-QAM: m = 0,
    S = 10 I, sums of small integers) and the trial is flagged SBCE_STATUS_DETECTOR by its second
    and third workgroup; nothing else is touched."""
    c, o, varn = lo.chunk_case(), lo.chunk_ref(kind), lo.CHUNK_VARN
    n_tx, n_rx, P, T_d, M = lo.CHUNK_SHAPE
    mom, st = _estep(sbce, c, varn, kind)
    bad = o["fail"]
    rat = lo.ratios({"moments": mom}, o, c["cons"], ok=~bad)["moments"]
    print(f"T_d 70 {kind}_soft: failed symbols {int(bad.sum())}, moments err / (eps kappa scale) "
          f"{rat:.3g} (bound {lo.C})")
    assert rat <= lo.C and np.all(np.isfinite(mom))
    assert bad.sum() == (T_d - lo.DEFECT_T0 if kind == "zf" else 0)
    assert list(st) == ([0, sbce._lib.SBCE_STATUS_DETECTOR, 0] if kind == "zf" else [0, 0, 0])
    cons = c["cons"]
    m_u, s_u = cons.sum() / M, (cons.real ** 2 + cons.imag ** 2).sum() / M
    assert m_u == 0 and s_u == 10
    uni = np.concatenate([np.full(n_tx, m_u), (s_u * np.eye(n_tx)).reshape(-1)])
    assert np.array_equal(mom[bad], np.broadcast_to(uni, (int(bad.sum()), uni.size)))


# ------------------------------------------------------------------ 2. the detector
@pytest.mark.parametrize("si,kind", [(3, "mmse"), (3, "zf"), (4, "mmse"), (6, "mmse"), (7, "zf")])
def test_estep_agrees_with_detect_linear(sbce, si, kind):
    """sbce_detect_linear with the EM posterior's sigma^2 = varn^2 and es = mean |cons|^2 gives
    the same moments (the two kernels share their solve; es is formed on the host there and on
    the device here, so the bound is the restatement's, not equal bits)."""
    c, varn = lo.case(si, 0), lo.VARNS[0]
    mom, _ = _estep(sbce, c, varn, kind)
    d = sbce.detect_linear_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], kind=kind,
                                 noise="em", es=float(np.mean(np.abs(c["cons"]) ** 2)),
                                 want=("moments",))["moments"]
    sc = lo.scales(lo.ref(si, 0, kind), c["cons"])["moments"]
    rat = float(np.max(np.abs(mom - d) / sc))
    print(f"shape {lo.SHAPES[si]} {kind}: vs sbce_detect_linear err / (eps kappa scale) {rat:.3g}")
    assert rat <= lo.C


# ------------------------------------------------------------------ 3. one stream
@pytest.mark.parametrize("vi", [0, 1])
def test_one_stream_zf_soft_is_the_soft_estep(sbce, vi):
    """n_tx = n_rx = 1: x_soft = y / h and nu = varn^2 / |h|^2, so |x_soft - c|^2 / nu is the
    exact posterior's exponent |y - h c|^2 / varn^2."""
    c, varn = lo.case(0, vi), lo.VARNS[vi]
    assert (c["n_tx"], c["y"].shape[2]) == (1, 1)
    mom, st = _estep(sbce, c, varn, "zf")
    m, S = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, 1, "soft")
    err = np.abs(mom - _moments(m, S)).max()
    print(f"varn {varn}: zf_soft vs soft moments, max abs difference {err:.2e}")
    assert not st.any() and err <= 1e-12


# ------------------------------------------------------------------ 4. chain parity
STATUS_BAD = 1 | 4 | 16 | 32        # NONHPD, DETECTOR, RANK, SINGULAR
EINVAL, EUNSUPPORTED = -1, -2       # include/sbce.h return codes


@pytest.mark.parametrize("shape,vi,kind", eo.CHAINS, ids=eo.chain_id)
def test_chain_parity_with_restated_loop(sbce, shape, vi, kind):
    c = eo.batch(shape, vi)
    r = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode=kind + "_soft", solve="chol")
    ref = eo.chain_ref(shape, vi, kind)
    errs = [rel(r["theta"][b], ref[b]["thetas"][-1]) for b in range(eo.B)]
    print(f"{shape} varn {c['varn']} {kind}_soft: theta rel err per trial "
          + " ".join(f"{e:.2e}" for e in errs) + f", status {r['status']}")
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert not (r["status"] & STATUS_BAD).any()
    assert max(errs) <= 1e-9


# ------------------------------------------------------------------ 5. noise, truth-free stop
def test_em_noise_matches_restated_loop(sbce):
    """(5, 6, 3, 20) MMSE, the parameter started at the generating varn = 0.3: theta and the
    parameter's history against noise_oracle's loop on the restated E-step."""
    shape, kind = eo.S56, "mmse"
    c = eo.batch(shape, 0)
    r = sbce.em_batch_noise(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode=kind + "_soft")
    ref = eo.noise_chain_ref(shape, 0, kind, eo.ITERS, c["varn"])
    e_th = max(rel(r["theta"][b], ref[b]["theta"]) for b in range(eo.B))
    e_h = np.abs(r["hist"] / np.stack([q["hist"] for q in ref]) - 1).max()
    print(f"em_noise {shape} {kind}_soft: theta {e_th:.3e} hist {e_h:.3e} varn {r['varn']}")
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert np.array_equal(r["varn"], r["hist"][:, -1])
    assert not r["status"].any() and not any(q["status"] for q in ref)
    assert e_th <= 1e-9 and e_h <= 1e-9


@pytest.mark.parametrize("shape,kind", [(eo.S56, "zf"), (eo.S88, "mmse")], ids=eo.chain_id)
def test_em_conv_that_cannot_stop_is_em_batch(sbce, shape, kind):
    """tol_theta = 0 with min_iters = max_iters: no rule can fire before the last iteration, and
    theta is bitwise em_batch's (the header's promise); n_tx = 5 and 8 are past sbce_loglik's
    limit, which only ll_hist keeps."""
    c = eo.batch(shape, 0)
    a = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode=kind + "_soft")
    r = sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], tol_theta=0.0,
                           min_iters=eo.ITERS, mode=kind + "_soft")
    assert np.array_equal(r["theta"], a["theta"])
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert np.all(np.isfinite(r["dtheta_hist"])) and r["ll_hist"] is None
    with pytest.raises(sbce.SbceError):                    # ll_hist keeps sbce_loglik's n_tx <= 4
        sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], loglik=True,
                           mode=kind + "_soft")


# ------------------------------------------------------------------ 6. independence
@pytest.mark.parametrize("shape,kind", [(eo.S56, "zf"), (eo.S88, "mmse"), (eo.S68, "mmse")],
                         ids=eo.chain_id)
def test_batch_independence_and_per_trial_variance(sbce, shape, kind):
    c = eo.batch(shape, 0)
    mode = kind + "_soft"
    full = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode=mode)
    one = sbce.em_batch(*_args(c, slice(1, 2)), c["varn"], eo.ITERS, c["theta0"][1:2], mode=mode)
    assert np.array_equal(full["theta"][1:2], one["theta"])
    vt = sbce.em_batch(*_args(c), np.full(eo.B, c["varn"]), eo.ITERS, c["theta0"], mode=mode)
    assert np.array_equal(vt["theta"], full["theta"])
    assert np.array_equal(vt["status"], full["status"])
    e = dict(y=c["y_d"], psi=c["psi_d"], cons=c["cons"], theta=c["theta0"], n_tx=c["n_tx"])
    mom, _ = _estep(sbce, e, c["varn"], kind)
    mom_t, _ = _estep(sbce, e, np.full(eo.B, c["varn"]), kind)
    mom_1, _ = _estep(sbce, {k: (v[1:2] if k in ("y", "psi", "theta") else v) for k, v in e.items()},
                      c["varn"], kind)
    assert np.array_equal(mom_t, mom) and np.array_equal(mom_1, mom[1:2])


# ------------------------------------------------------------------ 7. the `done` skip
def test_freeze_gives_the_bits_of_sbce_em(sbce):
    """(8, 8, 5, 48) MMSE with varn = 0.05 (saturating posteriors), 12 iterations: the batched
    Cholesky arms the fixed-point freeze, so the E-step kernel runs with EstepArgs::done set and
    skips whatever trial froze.  sbce_em_multi (n = 1) may end its launch sequence early; its
    theta and iters_done are sbce_em's bits either way.  Nothing is asserted about when, or
    whether, a trial freezes."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    c, iters, varn = eo.batch(eo.S88, 0), 12, 0.05
    a = sbce.em_batch(*_args(c), varn, iters, c["theta0"], mode="mmse_soft")
    st = em._Staged(torch, *_args(c), c["theta0"], varn, solve=em._SOLVES["chol"], check="theta0",
                    clone=True)
    ptrs = st.ptrs()
    L = sbce._lib
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    dims = (ctypes.POINTER(L.Dims) * 1)(ctypes.pointer(st.dims))
    pp = (ctypes.POINTER(L.Ptrs) * 1)(ctypes.pointer(ptrs))
    strs = (ctypes.c_void_p * 1)(stream.cuda_stream)
    issued = (ctypes.c_int * 1)(-1)
    rc = L.load().sbce_em_multi(1, dims, pp, iters, L.SBCE_ESTEP_MMSE_SOFT, L.SBCE_SOLVE_CHOL, strs,
                                0, issued)
    assert rc == 0, rc
    torch.cuda.synchronize()
    print(f"freeze: iters_issued {issued[0]} of {iters}, status {a['status']}")
    assert 1 <= issued[0] <= iters
    assert np.array_equal(st.theta.cpu().numpy(), a["theta"])
    assert np.array_equal(st.iters_done.cpu().numpy(), a["iters_done"])
    assert np.array_equal(a["iters_done"], np.full(eo.B, iters))
    assert np.all(np.isfinite(a["theta"]))


# ------------------------------------------------------------------ 8. graph capture
def test_graph_capture_replays_the_eager_bits(sbce):
    import torch
    c = eo.batch(eo.S56, 0)
    b = dict(y_d=c["y_d"], y_p=c["y_p"], psi_d=c["psi_d"], u_p=c["u_p"], cons=c["cons"],
             theta0=c["theta0"])
    eng = sbce.EMEngine(b, c["varn"], mode="mmse_soft")
    th = eng.run(3).cpu().numpy()
    it, st = eng.iters_done.cpu().numpy(), eng.status.cpu().numpy()
    g = eng.capture(3)
    for _ in range(2):
        eng.theta.fill_(float("nan"))
        eng.iters_done.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(eng.theta.cpu().numpy(), th)
        assert np.array_equal(eng.iters_done.cpu().numpy(), it)
        assert np.array_equal(eng.status.cpu().numpy(), st)
    assert np.isfinite(th).all()
    ref = eo.chain_ref(eo.S56, 0, "mmse")
    assert max(rel(th[i], ref[i]["thetas"][2]) for i in range(eo.B)) <= 1e-9


# ------------------------------------------------------------------ 9. error codes
def test_error_codes_before_any_launch(sbce):
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    c = eo.batch(eo.S34, 0)                                # n_tx 3, n_rx 4, P 2
    st = em._Staged(torch, *_args(c), c["theta0"], c["varn"], solve=L.SBCE_SOLVE_CHOL,
                    check="theta0", clone=True)
    before = st.theta.cpu().numpy().copy()
    xbuf = torch.zeros((eo.B, eo.T_D, 3), dtype=torch.complex128, device="cuda")
    mom = torch.full((eo.B, eo.T_D, 12), -7.0, dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    MM, ZF = L.SBCE_ESTEP_MMSE_SOFT, L.SBCE_ESTEP_ZF_SOFT

    def dims(**over):
        v = {f: getattr(st.dims, f) for f, _ in L.Dims._fields_}
        v.update(over)
        return L.Dims(*[v[f] for f, _ in L.Dims._fields_])

    def em_rc(d, mode, **ptr):
        return lib.sbce_em(d, st.ptrs(**ptr), 2, mode, L.SBCE_SOLVE_CHOL, stream)

    def estep_rc(d, mode):
        return lib.sbce_estep(d, st.ptrs(), mode, mom.data_ptr(), stream)

    wide = dims(n_tx=4, n_rx=3, n_psi=2)                   # n_rx < n_tx; K = 24 as staged
    assert em_rc(wide, ZF) == EUNSUPPORTED and estep_rc(wide, ZF) == EUNSUPPORTED
    nine = dims(n_tx=9, n_rx=8)
    for mode in (MM, ZF):
        assert em_rc(nine, mode) == EUNSUPPORTED
        assert estep_rc(nine, mode) == EUNSUPPORTED
        assert em_rc(dims(n_rx=9), mode) == EUNSUPPORTED
        assert em_rc(dims(m=12), mode) == EUNSUPPORTED      # not a power of two
        assert em_rc(st.dims, mode, x_dest=xbuf) == EINVAL
        assert em_rc(st.dims, mode, x_sup=xbuf) == EINVAL
    assert em_rc(nine, L.SBCE_ESTEP_PM_SOFT) == EINVAL      # every other mode: as before
    assert em_rc(st.dims, 9) == EUNSUPPORTED and estep_rc(st.dims, 9) == EUNSUPPORTED
    with pytest.raises(KeyError):
        sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="mmse_hard")
    torch.cuda.synchronize()
    assert np.array_equal(st.theta.cpu().numpy(), before)          # nothing was launched
    assert np.all(mom.cpu().numpy() == -7.0)
    assert em_rc(st.dims, MM) == 0 and estep_rc(st.dims, ZF) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(st.theta.cpu().numpy(), before)
    assert not np.any(mom.cpu().numpy() == -7.0)


def test_single_trial_front_ends(sbce):
    """em_mmse_soft / em_zf_soft (em_mmse's argument list; the (M,) table stands in for the
    hypothesis table) are trial 0 of em_batch."""
    c = eo.batch(eo.S56, 0)
    n_tx, n_rx, P, T_p, M = eo.S56
    Y_d, Y_p = [y[:, None] for y in c["y_d"][0]], [y[:, None] for y in c["y_p"][0]]
    Z_p = [np.kron(u[None, :], np.eye(n_rx)) for u in c["u_p"][0]]
    for fn, mode in ((sbce.em_mmse_soft, "mmse_soft"), (sbce.em_zf_soft, "zf_soft")):
        full = sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode=mode)
        th = fn(Y_d, Y_p, eo.T_D, T_p, Z_p, c["psi_d"][0].T, c["cons"], M, c["varn"], 2,
                c["theta0"][0].reshape(-1, 1), None)
        assert th.shape == (P * n_tx * n_rx, 1)
        assert np.array_equal(th.reshape(-1), full["theta"][0])
