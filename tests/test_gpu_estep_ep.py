"""GPU tier of expectation propagation (csrc/ep_solve.h, csrc/estep_linear.hip and the EP kind of
csrc/detect_linear.hip; SBCE_ESTEP_EP, SBCE_LINEAR_EP): sbce_estep's moments and every
sbce_detect_linear output against the NumPy restatement (tests/ep_oracle.py), one pass against the
soft MMSE kernels, bitwise determinism, the EM chain through sbce_em / sbce_em_multi /
sbce_em_noise / sbce_em_conv against the restated loop, the error codes and the Python front ends.

Bounds: decisions, counters and status exact (the CPU tier, tests/test_ep.py, asserts that no
branch of the parity cases can flip on rounding); each continuous output within its own
16 max(r_k, 1) eps kappa_t scale (none above C_EP = 16 max(r, 1); 16 for post and the moments),
r_k measured on the CPU against a 50-digit copy of the restatement (ep_oracle.C_BY_OUTPUT); the
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

pytestmark = pytest.mark.gpu

ALL = ("x_soft", "nu", "x_hat", "idx", "llr", "post", "moments", "status")
KEYS = ALL + ("err",)
CONT = {"x_soft", "nu", "post", "llr", "llr_maxlog", "moments"}
SWEEP = (5, 1)                      # (8,8,5,24,16) at varn 1.0: the passes swept over {1, 2, 5, 16}
EINVAL, EUNSUPPORTED = -1, -2       # include/sbce.h return codes
STATUS_BAD = 1 | 4 | 16 | 32        # NONHPD, DETECTOR, RANK, SINGULAR


def _moments(m, S):
    return np.concatenate([m, S.reshape(*m.shape[:2], -1)], axis=2)


def _estep(sbce, c, varn, passes=None, mode="ep"):
    m, S, st = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], mode=mode,
                                return_status=True, ep_passes=passes)
    return _moments(m, S), st


def _detect(sbce, c, varn, passes=None, kind="ep", **kw):
    kw.setdefault("labels", c["labels"])
    kw.setdefault("want", ALL)
    return sbce.detect_linear_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"],
                                    kind=kind if passes is None else (kind, passes), **kw)


def _args(c, sl=slice(None)):
    return c["y_d"][sl], c["y_p"][sl], c["psi_d"][sl], c["u_p"][sl], c["cons"]


def _check_parity(sbce, c, varn, o, passes, what, ok=None):
    """Both kernels against the restatement result `o`; returns the detector's outputs."""
    mom, st = _estep(sbce, c, varn, passes)
    r = _detect(sbce, c, varn, passes, x_d_true=c["x"])
    rm = _detect(sbce, c, varn, passes, maxlog=True, want=("llr",))
    rat = lo.ratios(dict(r, llr_maxlog=rm["llr"]), o, c["cons"], ok=ok)
    rat_e = lo.ratios({"moments": mom}, o, c["cons"], ok=ok)["moments"]
    print(f"{what} p {passes}: max kappa {o['kappa'][~o['fail']].max():.3g}, err / (eps kappa "
          f"scale): estep moments {rat_e:.3g}, " + ", ".join(f"{k} {v:.3g}" for k, v in rat.items())
          + " (bounds " + ", ".join(f"{k} {v:.3g}" for k, v in ep.C_BY_OUTPUT.items()) + ")")
    assert np.all(np.isfinite(mom))
    assert np.array_equal(r["idx"], o["idx"]) and r["idx"].dtype == np.int32
    assert np.array_equal(r["x_hat"], o["x_hat"])
    assert np.array_equal(r["err"], o["err"])
    assert np.array_equal(r["status"], o["status"])                     # SBCE_STATUS_NONHPD
    assert np.array_equal(st, 4 * o["status"])                          # SBCE_STATUS_DETECTOR
    assert set(rat) == CONT
    assert rat_e <= ep.C_BY_OUTPUT["moments"], rat_e
    for k, v in rat.items():
        assert v <= ep.C_BY_OUTPUT[k] <= ep.C_EP, (k, v)
    return r, rm, mom


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("si,vi", ep.CASES)
def test_parity_with_restatement(sbce, si, vi):
    """sbce_estep's moments and every sbce_detect_linear output, p = 5 (the default: passed as 0)."""
    c, varn, o = ep.case(si, vi), ep.VARNS[vi], ep.ref(si, vi)
    _check_parity(sbce, c, varn, o, None, f"shape {ep.SHAPES[si]} varn {varn}")


@pytest.mark.parametrize("passes", [1, 2, 5, 16])
def test_parity_over_the_pass_count(sbce, passes):
    si, vi = SWEEP
    c, varn, o = ep.case(si, vi), ep.VARNS[vi], ep.ref(si, vi, passes)
    r, _, mom = _check_parity(sbce, c, varn, o, passes, f"shape {ep.SHAPES[si]} varn {varn}")
    if passes == ep.PASSES:                                # 0 and 5 are the same launch
        assert np.array_equal(mom, _estep(sbce, c, varn, None)[0])
        assert np.array_equal(r["x_soft"], _detect(sbce, c, varn, None, want=("x_soft",))["x_soft"])


def test_several_workgroups_per_trial(sbce):
    """T_d = 70: three workgroups per trial, the last ragged.  Trial 1 (varn = 1e-8) loses a pivot
    on every symbol from 40 on: those carry the uniform posterior's outputs exactly (16-QAM:
    m = 0, S = 10 I, sums of small integers), the flag comes from the trial's second and third
    workgroup, and nothing else is touched: trial 1 of the batch is bitwise its B = 1 call."""
    c, o, varn = lo.chunk_case(), ep.chunk_ref(), np.array(ep.CHUNK_VARN_T)
    n_tx, n_rx, P, T_d, M = lo.CHUNK_SHAPE
    bad = o["fail"]
    r, rm, mom = _check_parity(sbce, c, varn, o, None, "T_d 70", ok=~bad)
    assert bad.sum() == T_d - lo.DEFECT_T0 and list(r["status"]) == [0, 1, 0]
    assert np.all(r["x_soft"][bad] == 0) and np.all(r["nu"][bad] == np.inf)
    assert np.all(r["post"][bad] == 1.0 / M) and np.all(r["llr"][bad] == 0)
    assert np.all(rm["llr"][bad] == 0)
    cons = c["cons"]
    m_u, s_u = cons.sum() / M, (cons.real ** 2 + cons.imag ** 2).sum() / M
    assert m_u == 0 and s_u == 10
    uni = np.concatenate([np.full(n_tx, m_u), (s_u * np.eye(n_tx)).reshape(-1)])
    for got in (mom, r["moments"]):
        assert np.array_equal(got[bad], np.broadcast_to(uni, (int(bad.sum()), uni.size)))
    one = sbce.detect_linear_batch(c["y"][1:2], c["psi"][1:2], cons, c["theta"][1:2],
                                   float(varn[1]), n_tx, kind="ep", labels=c["labels"],
                                   x_d_true=c["x"][1:2], want=ALL)
    for k in KEYS:
        assert np.array_equal(r[k][1:2], one[k]), k
    e1 = {k: (v[1:2] if k in ("y", "psi", "theta") else v) for k, v in c.items()}
    assert np.array_equal(_estep(sbce, e1, float(varn[1]))[0], mom[1:2])


# ------------------------------------------------------------------ 2. one pass is soft MMSE
@pytest.mark.parametrize("si,vi", [(1, 0), (3, 1), (4, 0), (5, 0), (6, 0)])
def test_one_pass_is_the_soft_mmse_kernel(sbce, si, vi):
    """p = 1 against mode 'mmse_soft' and kind 'mmse' on the device, within the MMSE bound.  Not
    asserted bitwise: the EP solve takes L[a][j] from the lane's own column entry."""
    c, varn = ep.case(si, vi), ep.VARNS[vi]
    o = lo.linear_ref(c["y"], c["psi"], c["cons"], c["theta"], varn * varn, c["n_tx"], kind="mmse",
                      labels=c["labels"])
    mom, st = _estep(sbce, c, varn, 1)
    mom_m, st_m = _estep(sbce, c, varn, None, mode="mmse_soft")
    r = _detect(sbce, c, varn, 1)
    r_m = _detect(sbce, c, varn, None, kind="mmse")
    sc = lo.scales(o, c["cons"])
    rat = {k: float(np.max(np.abs(r[k] - r_m[k]) / sc[k])) for k in ("x_soft", "nu", "post", "llr",
                                                                     "moments")}
    rat["estep"] = float(np.max(np.abs(mom - mom_m) / sc["moments"]))
    same = np.array_equal(mom, mom_m) and all(np.array_equal(r[k], r_m[k]) for k in ALL)
    print(f"shape {ep.SHAPES[si]} varn {varn}: p = 1 vs MMSE err / (eps kappa scale): "
          + ", ".join(f"{k} {v:.3g}" for k, v in rat.items()) + f" (bound {lo.C}); bitwise: {same}")
    assert np.array_equal(r["idx"], r_m["idx"]) and not st.any() and not st_m.any()
    assert max(rat.values()) <= lo.C


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("shape", [eo.S56, eo.S88, eo.S68], ids=eo.chain_id)
def test_batch_independence_and_per_trial_variance(sbce, shape):
    c = eo.batch(shape, 0)
    full = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep")
    one = sbce.em_batch(*_args(c, slice(1, 2)), c["varn"], eo.ITERS, c["theta0"][1:2], mode="ep")
    assert np.array_equal(full["theta"][1:2], one["theta"])
    vt = sbce.em_batch(*_args(c), np.full(eo.B, c["varn"]), eo.ITERS, c["theta0"], mode="ep")
    assert np.array_equal(vt["theta"], full["theta"])
    assert np.array_equal(vt["status"], full["status"])
    e = dict(y=c["y_d"], psi=c["psi_d"], cons=c["cons"], theta=c["theta0"], n_tx=c["n_tx"])
    mom, _ = _estep(sbce, e, c["varn"])
    mom_t, _ = _estep(sbce, e, np.full(eo.B, c["varn"]))
    mom_1, _ = _estep(sbce, {k: (v[1:2] if k in ("y", "psi", "theta") else v) for k, v in e.items()},
                      c["varn"])
    assert np.array_equal(mom_t, mom) and np.array_equal(mom_1, mom[1:2])


def test_detector_batch_independence_and_per_trial_sigma2(sbce):
    c = ep.case(3, 0)
    vt = np.array([0.1, 1.0, 0.3])
    r = _detect(sbce, c, vt, x_d_true=c["x"])
    for b in range(3):
        one = sbce.detect_linear_batch(c["y"][b:b + 1], c["psi"][b:b + 1], c["cons"],
                                       c["theta"][b:b + 1], float(vt[b]), c["n_tx"], kind="ep",
                                       labels=c["labels"], x_d_true=c["x"][b:b + 1], want=ALL)
        for k in KEYS:
            assert np.array_equal(r[k][b:b + 1], one[k]), (k, b)


def test_detector_graph_capture_replays_the_eager_bits(sbce):
    import torch
    em = import_module(sbce.__name__ + ".em")
    c = ep.case(4, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(c["x"])).cuda()
    args = (torch, *dev, c["n_tx"], "ep", 0.09, None, lo.default_es(c["cons"]), lab, xd, False, ALL, 3)
    eager = {k: v.cpu().numpy() for k, v in em._detect_linear_call(*args).items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()                                # one stream: the graph is a linear chain
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = em._detect_linear_call(*args)
    for _ in range(2):
        for v in out.values():
            v.fill_(1)
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert np.array_equal(out[k].cpu().numpy(), v), k
    o = ep.ref(4, 0, 3)
    assert np.array_equal(eager["idx"], o["idx"]) and np.array_equal(eager["err"], o["err"])


def _multi(sbce, c, varn, iters):
    """sbce_em_multi (n = 1) on a fresh staging of the batch: (theta, iters_done, iters_issued)."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    st = em._Staged(torch, *_args(c), c["theta0"], varn, solve=em._SOLVES["chol"], check="theta0",
                    clone=True)
    ptrs = st.ptrs()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    dims = (ctypes.POINTER(L.Dims) * 1)(ctypes.pointer(st.dims))
    pp = (ctypes.POINTER(L.Ptrs) * 1)(ctypes.pointer(ptrs))
    strs = (ctypes.c_void_p * 1)(stream.cuda_stream)
    issued = (ctypes.c_int * 1)(-1)
    rc = L.load().sbce_em_multi(1, dims, pp, iters, L.SBCE_ESTEP_EP, L.SBCE_SOLVE_CHOL, strs, 0,
                                issued)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return st.theta.cpu().numpy(), st.iters_done.cpu().numpy(), issued[0]


@pytest.mark.parametrize("varn,iters", [(0.3, eo.ITERS), (0.05, 12)])
def test_em_multi_and_the_freeze_give_the_bits_of_sbce_em(sbce, varn, iters):
    """(8, 8, 5, 48): the batched Cholesky arms the fixed-point freeze, so the EP kernel runs with
    EstepArgs::done set and skips whatever trial froze (varn = 0.05, 12 iterations: saturating
    posteriors); sbce_em_multi may end its launch sequence early.  Its theta and iters_done are
    sbce_em's bits either way.  Nothing is asserted about when, or whether, a trial freezes."""
    c = eo.batch(eo.S88, 0)
    a = sbce.em_batch(*_args(c), varn, iters, c["theta0"], mode="ep")
    theta, done, issued = _multi(sbce, c, varn, iters)
    print(f"varn {varn}: iters_issued {issued} of {iters}, status {a['status']}")
    assert 1 <= issued <= iters
    assert np.array_equal(theta, a["theta"]) and np.array_equal(done, a["iters_done"])
    assert np.array_equal(a["iters_done"], np.full(eo.B, iters))
    assert np.all(np.isfinite(a["theta"]))


def test_a_stopped_trial_keeps_its_moments(sbce):
    """sbce_em_conv with a loose theta rule stops the trials at different iterations and flags them
    in the `done` words the E-step reads.  The workspace begins with the moments: those of a trial
    that stopped after iteration k are the E-step's at theta_{k-1}, bit for bit -- no later launch
    rewrote them."""
    import torch
    em = import_module(sbce.__name__ + ".em")
    L = sbce._lib
    lib = L.load()
    c, iters = eo.batch(eo.S56, 1), 8                      # varn 1.0: the steps shrink slowly
    n_tx, T_d = c["n_tx"], eo.T_D
    st = em._Staged(torch, *_args(c), c["theta0"], c["varn"], solve=L.SBCE_SOLVE_CHOL,
                    check="theta0", clone=True)
    dth = torch.zeros((eo.B, iters), dtype=torch.float64, device="cuda")
    scratch = em._scratch(torch, lib.sbce_conv_workspace_bytes, "sbce_conv_workspace_bytes",
                          ctypes.byref(st.dims), 0)
    cv = L.ConvOpts(0.05, 0.0, 1, 0, dth.data_ptr(), None, scratch.data_ptr(), scratch.numel())
    rc = lib.sbce_em_conv(st.dims, st.ptrs(), iters, L.SBCE_ESTEP_EP, L.SBCE_SOLVE_CHOL, None,
                          ctypes.byref(cv), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    done = st.iters_done.cpu().numpy()
    MS = n_tx + n_tx * n_tx
    mom = st.ws[:eo.B * T_d * MS * 16].cpu().numpy().view(np.complex128).reshape(eo.B, T_d, MS)
    print(f"iters_done {done}, status {st.status.cpu().numpy()}")
    assert done.min() < iters and done.min() >= 1            # some trial did stop early
    for b in range(eo.B):
        k = int(done[b])
        th = c["theta0"] if k == 1 else sbce.em_batch(*_args(c), c["varn"], k - 1, c["theta0"],
                                                     mode="ep")["theta"]
        e = dict(y=c["y_d"][b:b + 1], psi=c["psi_d"][b:b + 1], cons=c["cons"], theta=th[b:b + 1],
                 n_tx=n_tx)
        assert np.array_equal(_estep(sbce, e, c["varn"])[0][0], mom[b]), b


# ------------------------------------------------------------------ 4. the chain
@pytest.mark.parametrize("shape", ep.CHAIN_SHAPES, ids=eo.chain_id)
def test_chain_parity_with_restated_loop(sbce, shape):
    c = eo.batch(shape, 0)
    r = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep", solve="chol")
    ref = ep.chain_ref(shape)
    errs = [rel(r["theta"][b], ref[b]["thetas"][-1]) for b in range(eo.B)]
    bars = [ref[b]["bar"] for b in range(eo.B)]
    print(f"{shape} varn {c['varn']} ep: theta rel err per trial "
          + " ".join(f"{e:.2e}" for e in errs) + "; bars " + " ".join(f"{v:.2e}" for v in bars)
          + f", status {r['status']}")
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert not (r["status"] & STATUS_BAD).any()
    assert max(bars) <= 1e-7
    for e, bar in zip(errs, bars):
        assert e <= bar


def test_em_noise_matches_restated_loop(sbce):
    """(5, 6, 3, 20), the parameter started at the generating varn = 0.3: theta and the parameter's
    history against noise_oracle's loop on the restated EP E-step."""
    shape = eo.S56
    c = eo.batch(shape, 0)
    r = sbce.em_batch_noise(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep")
    ref = ep.noise_chain_ref(shape, 0, eo.ITERS, c["varn"])
    e_th = max(rel(r["theta"][b], ref[b]["theta"]) for b in range(eo.B))
    e_h = np.abs(r["hist"] / np.stack([q["hist"] for q in ref]) - 1).max()
    print(f"em_noise {shape} ep: theta {e_th:.3e} hist {e_h:.3e} varn {r['varn']}")
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert np.array_equal(r["varn"], r["hist"][:, -1])
    assert not r["status"].any() and not any(q["status"] for q in ref)
    assert e_th <= 1e-9 and e_h <= 1e-9


@pytest.mark.parametrize("shape", [eo.S56, eo.S88], ids=eo.chain_id)
def test_em_conv_that_cannot_stop_is_em_batch(sbce, shape):
    """tol_theta = 0 with min_iters = max_iters: no rule can fire before the last iteration, and
    theta is bitwise em_batch's; n_tx = 5 and 8 are past sbce_loglik's limit, which only ll_hist
    keeps."""
    c = eo.batch(shape, 0)
    a = sbce.em_batch(*_args(c), c["varn"], eo.ITERS, c["theta0"], mode="ep")
    r = sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], tol_theta=0.0,
                           min_iters=eo.ITERS, mode="ep")
    assert np.array_equal(r["theta"], a["theta"])
    assert np.array_equal(r["iters_done"], np.full(eo.B, eo.ITERS))
    assert np.all(np.isfinite(r["dtheta_hist"])) and r["ll_hist"] is None
    with pytest.raises(sbce.SbceError):                    # ll_hist keeps sbce_loglik's n_tx <= 4
        sbce.em_batch_conv(*_args(c), c["varn"], eo.ITERS, c["theta0"], loglik=True, mode="ep")


# ------------------------------------------------------------------ 5. error codes
def test_estep_error_codes_before_any_launch(sbce):
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
    EP = L.SBCE_ESTEP_EP

    def dims(**over):
        v = {f: getattr(st.dims, f) for f, _ in L.Dims._fields_}
        v.update(over)
        return L.Dims(*[v[f] for f, _ in L.Dims._fields_])

    def em_rc(d, **ptr):
        return lib.sbce_em(d, st.ptrs(**ptr), 2, EP, L.SBCE_SOLVE_CHOL, stream)

    def estep_rc(d):
        return lib.sbce_estep(d, st.ptrs(), EP, mom.data_ptr(), stream)

    nine = dims(n_tx=9, n_rx=8)
    assert em_rc(nine) == EUNSUPPORTED and estep_rc(nine) == EUNSUPPORTED
    assert em_rc(dims(n_rx=9)) == EUNSUPPORTED and estep_rc(dims(n_rx=9)) == EUNSUPPORTED
    assert em_rc(dims(m=12)) == EUNSUPPORTED and estep_rc(dims(m=12)) == EUNSUPPORTED
    assert em_rc(dims(partition_r=17)) == EINVAL and estep_rc(dims(partition_r=17)) == EINVAL
    assert em_rc(st.dims, x_dest=xbuf) == EINVAL
    assert em_rc(st.dims, x_sup=xbuf) == EINVAL
    with pytest.raises(KeyError):
        sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep_soft")
    torch.cuda.synchronize()
    assert np.array_equal(st.theta.cpu().numpy(), before)          # nothing was launched
    assert np.all(mom.cpu().numpy() == -7.0)
    assert estep_rc(dims(partition_r=16)) == 0 and em_rc(st.dims) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(st.theta.cpu().numpy(), before)
    assert not np.any(mom.cpu().numpy() == -7.0)


def test_detector_error_codes_before_any_launch(sbce):
    import torch
    L = sbce._lib
    lib = L.load()
    c = ep.case(1, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    out = torch.full((3, 5, 2), -7.0, dtype=torch.float64, device="cuda")

    def call(**over):
        v = dict(batch=3, n_tx=2, n_rx=2, n_psi=3, t_d=5, m=16, kind=L.SBCE_LINEAR_EP, flags=0,
                 sigma2=0.09, es=10.0)
        v.update(over)
        d = L.LinearDims(*[v[f] for f, _ in L.LinearDims._fields_])
        p = L.LinearPtrs(y_d=dev[0].data_ptr(), psi_d=dev[1].data_ptr(), cons=dev[2].data_ptr(),
                         theta=dev[3].data_ptr(), nu=out.data_ptr())
        return lib.sbce_detect_linear(d, p, torch.cuda.current_stream().cuda_stream)

    assert call(n_tx=9, n_rx=8) == EUNSUPPORTED and call(n_rx=9) == EUNSUPPORTED
    assert call(flags=L.linear_ep_passes(17)) == EINVAL
    assert call(flags=L.linear_ep_passes(3), kind=L.SBCE_LINEAR_MMSE) == EINVAL
    assert call(flags=L.linear_ep_passes(3), kind=L.SBCE_LINEAR_ZF) == EINVAL
    assert call(flags=1 << 16) == EINVAL and call(flags=2) == EINVAL
    assert call(es=0.0) == EINVAL and call(kind=2) == EINVAL and call(m=12) == EINVAL
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)               # nothing was launched
    assert call(flags=L.linear_ep_passes(16) | L.SBCE_DETECT_MAXLOG) == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() > 0)


# ------------------------------------------------------------------ 6. Python front ends
def test_python_front_ends(sbce):
    c = eo.batch(eo.S56, 0)
    n_tx, n_rx, P, T_p, M = eo.S56
    Y_d, Y_p = [y[:, None] for y in c["y_d"][0]], [y[:, None] for y in c["y_p"][0]]
    Z_p = [np.kron(u[None, :], np.eye(n_rx)) for u in c["u_p"][0]]
    for passes in (None, 2):
        full = sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep", ep_passes=passes)
        th = sbce.em_ep(Y_d, Y_p, eo.T_D, T_p, Z_p, c["psi_d"][0].T, c["cons"], M, c["varn"], 2,
                        c["theta0"][0].reshape(-1, 1), None, ep_passes=passes)
        assert th.shape == (P * n_tx * n_rx, 1)
        assert np.array_equal(th.reshape(-1), full["theta"][0])
    two = sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep", ep_passes=2)["theta"]
    assert not np.array_equal(two, sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep")["theta"])
    b = dict(y_d=c["y_d"], y_p=c["y_p"], psi_d=c["psi_d"], u_p=c["u_p"], cons=c["cons"],
             theta0=c["theta0"])
    eng = sbce.EMEngine(b, c["varn"], mode="ep", ep_passes=2, x_d_true=c["x_d"])
    assert np.array_equal(eng.run(2).cpu().numpy(), two)
    d = eng.detect_linear(kind="ep", ep_passes=3, want=("x_soft", "idx"))
    d2 = sbce.detect_linear_batch(c["y_d"], c["psi_d"], c["cons"], two, c["varn"], n_tx,
                                  kind=("ep", 3), x_d_true=c["x_d"], want=("x_soft", "idx"))
    for k in ("x_soft", "idx", "err"):
        assert np.array_equal(d[k], d2[k]), k
    one = sbce.detect_linear([y[:, None] for y in c["y_d"][0]], c["psi_d"][0].T, c["cons"], M,
                             c["varn"], two[0].reshape(-1, 1), kind="ep", ep_passes=3,
                             want=("x_soft",))
    assert np.array_equal(one["x_soft"], d2["x_soft"][0])
    with pytest.raises(KeyError):
        sbce.estep_batch(c["y_d"], c["psi_d"], c["cons"], two, c["varn"], n_tx, mode="EP")
    with pytest.raises(ValueError):
        sbce.detect_linear_batch(c["y_d"], c["psi_d"], c["cons"], two, c["varn"], n_tx, kind="EP")
    with pytest.raises(ValueError):
        sbce.detect_linear_batch(c["y_d"], c["psi_d"], c["cons"], two, c["varn"], n_tx,
                                 kind=("mmse", 3))
    with pytest.raises(ValueError):
        sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="mmse_soft", ep_passes=2)
    for bad in (17, 256, 257, -1):                         # rejected before anything is packed
        with pytest.raises(ValueError):
            sbce.em_batch(*_args(c), c["varn"], 2, c["theta0"], mode="ep", ep_passes=bad)
        with pytest.raises(ValueError):
            sbce.detect_linear_batch(c["y_d"], c["psi_d"], c["cons"], two, c["varn"], n_tx,
                                     kind=("ep", bad))
