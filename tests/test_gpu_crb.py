"""GPU tier of the Cramer-Rao bounds: sbce_crb (csrc/crb.hip) against the NumPy oracle on every
build route and tile count up to the limit L = 512, on given and pilot-only moments, the pivot
rule, and the properties the interface promises (batch and workspace independence, sigma2
scaling, inputs untouched, graph capture, the sweep's bound curve)."""
import ctypes

import numpy as np
import pytest

import crb_oracle as orc

pytestmark = pytest.mark.gpu

# (n_tx, n_rx, P, T_p, T_d, M), all with T_p + T_d >= L.  L = 8: less than one tile; 15: one ragged
# tile, the n_tx = 3 build; 34: the small-M-step build route, ragged; 68: just past the small route,
# MFMA build, remainder of 4; 72: the n_tx = 8 build; 260: the headline shape, 16 tiles + 4; 512:
# the limit, 32 full tiles.
S8, S15, S34, S68, S72, S260, S512 = ((1, 2, 8, 8, 30, 16), (3, 5, 5, 12, 33, 4), (2, 2, 17, 16, 40, 4),
                                      (4, 4, 17, 16, 96, 4), (8, 8, 9, 8, 96, 4),
                                      (4, 4, 65, 16, 256, 16), (8, 2, 64, 16, 640, 4))
SHAPES = [S8, S15, S34, S68, S72, S260, S512]
VARN = 0.3
NONHPD = 1
_cache = {}
_id = lambda s: "x".join(map(str, s))


def _batch(sbce, shape, B=None):
    B = B or (2 if shape == S512 else 3)
    key = (shape, B)
    if key not in _cache:
        n_tx, n_rx, P, T_p, T_d, M = shape
        _cache[key] = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, VARN,
                                                        seed=31, pinv="scipy")
    return _cache[key]


def _args(b, sl=slice(None)):
    return b["y_d"][sl], b["y_p"][sl], b["psi_d"][sl], b["u_p"][sl], b["cons"], b["n_tx"]


def _genie(sbce, shape):
    """crb_batch(kind='genie') of the shape's batch, computed once."""
    key = ("genie", shape)
    if key not in _cache:
        b = _batch(sbce, shape)
        _cache[key] = sbce.crb_batch(*_args(b), VARN, kind="genie", x_d_true=b["x_d"])
    return _cache[key]


def _check(got, u_p, psi_d, S, n_rx, sigma2, what):
    """The parity rule of the cfg1-shape solves: relative error of tr_inv, and absolute error of
    diag_inv over max_l (R^-1)_ll, at most max(1e-9, 1e-13 cond(R)).  Returns the worst ratio."""
    worst = 0.0
    for i in range(len(u_p)):
        ref = orc.crb_reduced(u_p[i], psi_d[i], S[i], n_rx, sigma2)
        assert ref["identifiable"], (what, i)
        tol = max(1e-9, 1e-13 * ref["cond"])
        e_tr = abs(got["tr_inv"][i] - ref["tr_inv"]) / ref["tr_inv"]
        e_d = np.abs(got["diag_inv"][i] - ref["diag_inv"]).max() / ref["diag_inv"].max()
        e_m = abs(got["mse"][i] - ref["mse"]) / ref["mse"]
        print(f"{what} trial {i}: cond {ref['cond']:.3g} tr_inv {e_tr:.2e} diag_inv {e_d:.2e} "
              f"mse {e_m:.2e} (tol {tol:.1e})")
        worst = max(worst, e_tr / tol, e_d / tol, e_m / tol)
        assert got["status"][i] == 0
    return worst


# ------------------------------------------------------------------ 1. genie against the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_genie_matches_oracle(sbce, shape):
    b = _batch(sbce, shape)
    got = _genie(sbce, shape)
    assert got["tr_inv"].shape == (b["y_d"].shape[0],) and got["diag_inv"].shape[1] == shape[0] * shape[2]
    worst = _check(got, b["u_p"], b["psi_d"], orc.genie_S(b["x_d"]), shape[1], VARN, _id(shape))
    print(f"{_id(shape)}: worst error / tolerance {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. given moments, the engine
@pytest.mark.parametrize("shape", [S8, S15, S34, S68, S72], ids=_id)
def test_estep_moments_match_oracle_and_engine(sbce, shape):
    """The E-step's moments at theta_0, read back from the device, through kind='moments' against
    the oracle on the same moments; EMEngine.crb('em') is that call on the engine's own moments,
    bit for bit.  (em <= genie is not asserted: a soft S_t can exceed rank 1 either way.)"""
    n_tx, n_rx = shape[:2]
    mode = "soft" if n_tx <= 4 else "mmse_soft"
    b = _batch(sbce, shape)
    m, S = sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], b["theta0"], VARN, n_tx, mode=mode)
    got = sbce.crb_batch(*_args(b), VARN, kind="moments", m=m, S=S)
    worst = _check(got, b["u_p"], b["psi_d"], S, n_rx, VARN, _id(shape) + " " + mode)
    print(f"{_id(shape)}: worst error / tolerance {worst:.3g}")
    assert worst <= 1.0
    eng = sbce.EMEngine(b, VARN, mode=mode)
    th0 = eng.theta.cpu().numpy().copy()
    e = eng.crb("em")
    assert np.array_equal(eng.theta.cpu().numpy(), th0)
    mom = eng.mom.cpu().numpy()
    B, T_d = mom.shape[:2]
    ref = sbce.crb_batch(*_args(b), VARN, kind="moments", m=mom[..., :n_tx],
                         S=mom[..., n_tx:].reshape(B, T_d, n_tx, n_tx), h_true=b["h"])
    for k in ("tr_inv", "diag_inv", "mse", "bound", "status"):
        assert np.array_equal(e[k], ref[k]), k
    assert np.all(np.isfinite(e["bound"])) and np.all(e["bound"] > 0)


# ------------------------------------------------------------------ 3. pilot-only, finite
@pytest.mark.parametrize("n_tx,P", [(2, 5), (4, 17)])
def test_pilot_only_bound_with_identifying_pilots(sbce, n_tx, P):
    """Pilots that identify the channel on their own: u_p = psi_p (x) x_p with uniform random
    phases (psi[:, 0] = 1), 4-QAM symbols and T_p = 2 L."""
    L, B, n_rx, T_d = n_tx * P, 3, 2, 4
    g = np.random.default_rng(31)
    cons = sbce.qam.qam_constellation(4)
    psi_p = np.exp(2j * np.pi * g.uniform(size=(B, 2 * L, P)))
    psi_p[:, :, 0] = 1
    x_p = cons[g.integers(0, 4, (B, 2 * L, n_tx))]
    u_p = np.einsum("btp,bta->btpa", psi_p, x_p).reshape(B, 2 * L, L)
    psi_d = np.exp(2j * np.pi * g.uniform(size=(B, T_d, P)))
    got = sbce.crb_batch(None, np.zeros((B, 2 * L, n_rx), complex), psi_d, u_p, cons, n_tx, VARN,
                         kind="pilot")
    worst = _check(got, u_p, psi_d, np.zeros((B, T_d, n_tx, n_tx)), n_rx, VARN, f"pilot L={L}")
    print(f"pilot L={L}: worst error / tolerance {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 4. unidentifiable trials
def _all_inf(got, i):
    return (np.isposinf(got["tr_inv"][i]) and np.isposinf(got["mse"][i])
            and np.all(np.isposinf(got["diag_inv"][i])) and got["status"][i] & NONHPD)


def test_pilot_only_bound_of_the_dft_pilots_is_infinite(sbce):
    """The package's dft_n pilots have a zero last row: they never identify the channel."""
    b = _batch(sbce, S68)
    got = sbce.crb_batch(*_args(b), VARN, kind="pilot", h_true=b["h"])
    for i in range(3):
        ref = orc.crb_reduced(b["u_p"][i], b["psi_d"][i], np.zeros((S68[4], 4, 4)), 4, VARN)
        assert not ref["identifiable"]
        assert _all_inf(got, i) and np.isposinf(got["bound"][i]), i


def test_genie_bound_with_fewer_observations_than_unknowns_is_infinite(sbce):
    shape = (4, 4, 17, 16, 48, 4)                       # L = 68 against 64 observations
    b = _batch(sbce, shape)
    got = sbce.crb_batch(*_args(b), VARN, kind="genie", x_d_true=b["x_d"])
    for i in range(3):
        ref = orc.crb_reduced(b["u_p"][i], b["psi_d"][i], orc.genie_S(b["x_d"][i]), 4, VARN)
        assert not ref["identifiable"]
        assert _all_inf(got, i), i


def test_one_unidentifiable_trial_leaves_the_others_alone(sbce):
    b = _batch(sbce, S68)
    psi = b["psi_d"].copy()
    psi[1, :, :] = psi[1, 0, :]                         # one phase vector for every data symbol
    assert not orc.crb_reduced(b["u_p"][1], psi[1], orc.genie_S(b["x_d"][1]), 4, VARN)["identifiable"]
    got = sbce.crb_batch(b["y_d"], b["y_p"], psi, b["u_p"], b["cons"], 4, VARN, kind="genie",
                         x_d_true=b["x_d"])
    ref = _genie(sbce, S68)
    assert _all_inf(got, 1)
    for i in (0, 2):
        for k in ("tr_inv", "diag_inv", "mse", "status"):
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("shape", [S34, S68, S260], ids=_id)
def test_trial_bits_depend_on_neither_batch_nor_workspace(sbce, shape):
    b = _batch(sbce, shape)
    ref = _genie(sbce, shape)
    for i in range(3):
        sl = slice(i, i + 1)
        one = sbce.crb_batch(*_args(b, sl), VARN, kind="genie", x_d_true=b["x_d"][sl])
        for k in ("tr_inv", "diag_inv", "mse"):
            assert np.array_equal(one[k][0], ref[k][i]), (i, k)
    for fill in (0x00, 0xFF):
        got = sbce.crb_batch(*_args(b), VARN, kind="genie", x_d_true=b["x_d"], ws_fill=fill)
        for k in ("tr_inv", "diag_inv", "mse", "status"):
            assert np.array_equal(got[k], ref[k]), (fill, k)


# ------------------------------------------------------------------ 6. scaling
def test_sigma2_scales_mse_and_bound_only(sbce):
    b = _batch(sbce, S34)
    ref = _genie(sbce, S34)
    s2 = np.array([0.1, 0.3, 1.0])
    got = sbce.crb_batch(*_args(b), s2, kind="genie", x_d_true=b["x_d"], h_true=b["h"])
    assert np.array_equal(got["tr_inv"], ref["tr_inv"])
    assert np.array_equal(got["diag_inv"], ref["diag_inv"])
    mse = S34[1] * s2 * got["tr_inv"]
    bound = mse / np.sum(np.abs(b["h"]) ** 2, axis=1)
    assert np.abs(got["mse"] / mse - 1).max() <= 1e-14
    assert np.abs(got["bound"] / bound - 1).max() <= 1e-14


# ------------------------------------------------------------------ 7, 8. raw calls
def _raw(sbce, shape):
    """A sbce_crb call on buffers the test owns: (call, inputs dict, outputs dict)."""
    import torch
    L_ = sbce._lib
    lib = L_.load()
    n_tx, n_rx, P, T_p, T_d, M = shape
    b = _batch(sbce, shape)
    B = b["y_d"].shape[0]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex128)).cuda()
    m, S = sbce.genie_moments(b["x_d"])
    mom = np.concatenate([m, S.reshape(B, T_d, n_tx * n_tx)], axis=2)
    inp = dict(y_d=dev(b["y_d"]), y_p=dev(b["y_p"]), psi_d=dev(b["psi_d"]), u_p=dev(b["u_p"]),
               cons=dev(b["cons"]), theta=dev(b["theta0"]), moments=dev(mom), h=dev(b["h"]))
    dims = L_.Dims(B, n_tx, n_rx, P, T_p, T_d, M, 0, VARN, 1.0)
    ws = torch.zeros(L_.workspace_bytes(dims, L_.SBCE_SOLVE_CHOL), dtype=torch.uint8, device="cuda")
    nb = ctypes.c_size_t(0)
    L_.check(lib.sbce_crb_workspace_bytes(ctypes.byref(dims), ctypes.byref(nb)), "bytes")
    scratch = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    out = dict(tr_inv=f64(B), diag_inv=f64(B, n_tx * P), mse=f64(B), bound=f64(B),
               status=torch.zeros(B, dtype=torch.int32, device="cuda"))
    ptrs = L_.Ptrs(y_d=inp["y_d"].data_ptr(), y_p=inp["y_p"].data_ptr(),
                   psi_d=inp["psi_d"].data_ptr(), u_p=inp["u_p"].data_ptr(),
                   cons=inp["cons"].data_ptr(), theta=inp["theta"].data_ptr(),
                   h_true=inp["h"].data_ptr(), status=out["status"].data_ptr(),
                   workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    opts = L_.CrbOpts(VARN, None, out["tr_inv"].data_ptr(), out["diag_inv"].data_ptr(),
                      out["mse"].data_ptr(), out["bound"].data_ptr(), scratch.data_ptr(),
                      scratch.numel(), 0)

    def call():
        L_.check(lib.sbce_crb(dims, ptrs, inp["moments"].data_ptr(), opts,
                              torch.cuda.current_stream().cuda_stream), "sbce_crb")

    return call, inp, out, (ws, scratch)


@pytest.mark.parametrize("shape", [S34, S68], ids=_id)
def test_inputs_are_not_written(sbce, shape):
    import torch
    call, inp, out, _ = _raw(sbce, shape)
    before = {k: v.cpu().numpy().copy() for k, v in inp.items()}
    call()
    torch.cuda.synchronize()
    for k, v in inp.items():
        assert np.array_equal(v.cpu().numpy(), before[k]), k
    ref = _genie(sbce, shape)
    for k in ("tr_inv", "diag_inv", "mse"):
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k


def test_graph_capture_replays_the_eager_bits(sbce):
    import torch
    call, _, out, (ws, scratch) = _raw(sbce, S34)
    call()
    torch.cuda.synchronize()
    eager = {k: v.cpu().numpy().copy() for k, v in out.items()}
    assert np.all(np.isfinite(eager["bound"])) and np.all(eager["tr_inv"] > 0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    for v in list(out.values()) + [ws, scratch]:
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert np.array_equal(v.cpu().numpy(), eager[k]), k


# ------------------------------------------------------------------ 9. the sweep
def test_sweep_carries_the_genie_bound(sbce):
    kw = dict(SNR=(10,), T_d=50, T_p=12, N=10, monte_iter=4, itera=2, modes=("soft",))
    x, plain = sbce.sweeps.nmse_vs_snr(**kw)
    x2, curves, status = sbce.sweeps.nmse_vs_snr(bounds=True, return_status=True, **kw)
    assert set(plain) == {"soft"} and set(curves) == {"soft", "crb_genie"}
    assert np.array_equal(curves["soft"], plain["soft"])            # bit for bit
    c = curves["crb_genie"]
    print(f"soft {curves['soft']}, crb_genie {c}")
    assert c.shape == (1,) and np.isfinite(c[0]) and c[0] > 0      # L = 22 against 62 observations
    assert status["crb_genie"][0] == 0
