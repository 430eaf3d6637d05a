"""GPU tier of the noise-variance estimation: sbce_noise_var (csrc/noise.hip) against the NumPy
restatement at every kernel path, sbce_em_noise against the restated loop, and the properties the
interface promises (start-independent fixed point, batch independence, per-trial starts, floor,
early stop, no interference with sbce_em, graph capture)."""
import ctypes

import numpy as np
import pytest

from conftest import rel
import noise_oracle as orc

pytestmark = pytest.mark.gpu

# (n_tx, n_rx, P, T_p, T_d, M).  (3, 5, ..., 33): odd antenna count, ragged T_d, symbols that
# straddle a wave; (4, 4, 33, ...): two blocks per trial and more than one theta tile; (8, 8, 70,
# ...): nine theta tiles, a last tile of 6 phases.
SHAPES = [(1, 2, 8, 8, 30, 16), (2, 2, 8, 16, 40, 4), (2, 4, 8, 16, 40, 16), (3, 5, 5, 12, 33, 4),
          (4, 4, 4, 16, 48, 4), (4, 4, 33, 16, 64, 4), (8, 8, 3, 16, 24, 4), (8, 8, 70, 8, 20, 4)]
S22, S24, S88 = SHAPES[1], SHAPES[2], SHAPES[6]
S44W = SHAPES[5]
TRUE_VAR, START = 0.3, 1.0
_cache = {}


def _batch(sbce, shape, B, seed, varn=TRUE_VAR, varh=1.0):
    key = (shape, B, seed, varn, varh)
    if key not in _cache:
        n_tx, n_rx, P, T_p, T_d, M = shape
        _cache[key] = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, varn,
                                                        seed=seed, pinv="scipy", varh=varh)
    return _cache[key]


def _args(b, sl=slice(None)):
    return b["y_d"][sl], b["y_p"][sl], b["psi_d"][sl], b["u_p"][sl]


def _ref(b, i, itera, start, mode="soft", partition_r=0, varn_min=1e-6, h=None):
    """em_noise_ref of trial i, computed once per (batch, arguments)."""
    key = ("ref", id(b), i, itera, start, mode, partition_r, varn_min, h is not None)
    if key not in _cache:
        _cache[key] = orc.em_noise_ref(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T,
                                       b["cons"], start, itera, b["theta0"][i], b["n_tx"], mode,
                                       partition_r, varn_min, h)
    return _cache[key]


# ------------------------------------------------------------------ stand-alone kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_var_matches_restatement(sbce, shape):
    """sbce_noise_var on the restatement's theta and moments.  |d sigma^2| <= 1e-12 (sum ||y||^2
    + Q) / (n_rx (T_p + T_d)): every residual entry stands behind L + 2 rounded products."""
    n_tx, n_rx, P, T_p, T_d, M = shape
    B = 3
    b = _batch(sbce, shape, B, seed=31)
    mode, pr = ("soft", 0) if n_tx <= 4 else ("pm_soft", 1)
    ms, Ss, th = [], [], []
    for i in range(B):
        Psi = b["psi_d"][i].T
        m, S = orc.moments(b["theta0"][i], b["y_d"][i], Psi, b["cons"], START, n_tx, mode, pr)
        theta = b["theta0"][i]
        if T_p + n_tx * T_d >= 2 * P * n_tx:           # a determined M-step: use its theta
            R, rhs = orc.mstep_build(b["u_p"][i], b["y_p"][i], Psi, b["y_d"][i], m, S)
            theta = orc.mstep_solve(R, rhs)
        ms.append(m), Ss.append(S), th.append(theta)
    got = sbce.noise_var_batch(*_args(b), np.stack(th), np.stack(ms), np.stack(Ss), varn_min=1e-9)
    worst = 0.0
    for i in range(B):
        s2, Q, yy = orc.noise_var_ref(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, th[i],
                                      ms[i], Ss[i], parts=True)
        bound = 1e-12 * (yy + Q) / (n_rx * (T_p + T_d))
        worst = max(worst, abs(got[i] - s2) / bound)
    print(f"noise_var {shape}: |d sigma^2| / bound = {worst:.3e}")
    assert worst <= 1.0


# ------------------------------------------------------------------ full loop
LOOP_CASES = ([(s, "soft", 0) for s in SHAPES if s[0] <= 4]
              + [(S24, "hard", 0), (S88, "pm_soft", 1), (S22, "zf", 0)])


@pytest.mark.parametrize("shape,mode,pr", LOOP_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_em_noise_matches_restated_loop(sbce, shape, mode, pr):
    """5 iterations from varn = 1.0 on data of true variance 0.3: theta, varn and hist at the
    rtol 1e-9 of the project's driver fixtures.

    (4, 4, 33, 16, 64, 4) has L = 132 unknowns per antenna against T_p + T_d = 80 observations:
    the channel can fit every observation of a hardened posterior exactly, R is then singular and
    sigma^2 runs to its floor.  With unit-variance channels (varh = 1) that happens in the FIRST
    iteration: cond R = 1e11..1e14, then 1e17, the restatement's np.linalg.solve returns rounding
    noise while the device drops the dead pivots (SBCE_STATUS_NONHPD), and a first run measured
    theta 1.9 relative, hist 4.1e-5 relative apart, varn equal (both at the floor, status 65).
    There is nothing to compare there, so this shape's channels are drawn with varh = 0.05: the
    posterior stays soft for the five iterations (cond R <= 5e5 in the restatement) and the
    comparison is one of the arithmetic, at the same bar."""
    B = 4
    b = _batch(sbce, shape, B, seed=41, varh=0.05 if shape == S44W else 1.0)
    r = sbce.em_batch_noise(*_args(b), b["cons"], START, 5, b["theta0"], mode=mode, partition_r=pr)
    refs = [_ref(b, i, 5, START, mode, pr) for i in range(B)]
    e_th = max(rel(r["theta"][i], refs[i]["theta"]) for i in range(B))
    ref_v = np.array([q["varn"] for q in refs])
    ref_h = np.stack([q["hist"] for q in refs])
    e_v = np.abs(r["varn"] / ref_v - 1).max()
    e_h = np.abs(r["hist"] / ref_h - 1).max()
    print(f"em_noise {shape} {mode}: theta {e_th:.3e} varn {e_v:.3e} hist {e_h:.3e} "
          f"sigma2 {r['sigma2']} status {r['status']}")
    assert np.array_equal(r["sigma2"], r["varn"] ** 2)
    assert np.array_equal(r["iters_done"], np.full(B, 5))
    assert np.array_equal(r["varn"], r["hist"][:, -1])
    assert e_v <= 1e-9 and e_h <= 1e-9
    assert e_th <= 1e-9


def test_underdetermined_shape_runs_to_the_floor(sbce):
    """L > T_p + T_d with unit-variance channels (see above): the likelihood is unbounded in
    sigma^2 -> 0, and both the restatement and the device end at varn_min, flagged, theta finite."""
    B = 4
    b = _batch(sbce, S44W, B, seed=41)
    L = sbce._lib
    r = sbce.em_batch_noise(*_args(b), b["cons"], START, 5, b["theta0"])
    for i in range(B):
        ref = _ref(b, i, 5, START)
        assert ref["varn"] == 1e-6 and ref["status"] == 64
    assert np.all(r["varn"] == 1e-6) and np.all(r["status"] & L.SBCE_STATUS_NOISE)
    assert np.all(np.isfinite(r["theta"])) and np.all(np.isfinite(r["hist"]))


# ------------------------------------------------------------------ further checks
def test_fixed_point_does_not_depend_on_the_start(sbce):
    B = 3
    b = _batch(sbce, S22, B, seed=21)
    for i in range(B):                                  # the restatement first, on this seed
        lo, hi = _ref(b, i, 12, 0.1)["varn"] ** 2, _ref(b, i, 12, 3.0)["varn"] ** 2
        assert abs(lo - hi) <= 1e-6 * hi, (i, lo, hi)
    lo = sbce.em_batch_noise(*_args(b), b["cons"], 0.1, 12, b["theta0"])["sigma2"]
    hi = sbce.em_batch_noise(*_args(b), b["cons"], 3.0, 12, b["theta0"])["sigma2"]
    print("fixed point sigma2:", lo, hi, np.abs(lo / hi - 1).max())
    assert np.all(np.abs(lo - hi) <= 1e-6 * hi)
    assert np.all(lo < TRUE_VAR * 1.5) and np.all(lo > TRUE_VAR * 0.3)


def test_trial_is_bitwise_independent_of_the_batch(sbce):
    shape = SHAPES[5]                                   # two blocks per trial
    b = _batch(sbce, shape, 37, seed=51)
    big = sbce.em_batch_noise(*_args(b), b["cons"], START, 3, b["theta0"])
    for i in (0, 18, 36):
        sl = slice(i, i + 1)
        one = sbce.em_batch_noise(*_args(b, sl), b["cons"], START, 3, b["theta0"][sl])
        for k in ("theta", "varn", "hist", "status"):
            assert np.array_equal(big[k][sl], one[k]), (i, k)


def test_per_trial_start_values(sbce):
    B = 4
    b = _batch(sbce, S22, B, seed=41)
    starts = np.array([0.2, 0.6, 1.0, 2.5])
    r = sbce.em_batch_noise(*_args(b), b["cons"], starts, 2, b["theta0"])
    same = sbce.em_batch_noise(*_args(b), b["cons"], START, 2, b["theta0"])
    for i in range(B):
        sl = slice(i, i + 1)
        one = sbce.em_batch_noise(*_args(b, sl), b["cons"], float(starts[i]), 2, b["theta0"][sl])
        assert np.array_equal(r["hist"][sl], one["hist"]) and np.array_equal(r["theta"][sl], one["theta"])
        ref = _ref(b, i, 2, float(starts[i]))
        assert np.allclose(r["hist"][i], ref["hist"], rtol=1e-9, atol=0)
    assert np.array_equal(r["hist"][2], same["hist"][2])
    assert not np.array_equal(r["hist"][0, 0], same["hist"][0, 0])


def _floor_batch(sbce):
    """Trial 0 noiseless, trial 1 with noise variance 0.3; random full-rank pilots, T_p >= L."""
    g = np.random.default_rng(2)
    n_tx = n_rx = 2
    P, T_p, T_d = 4, 12, 30
    L = P * n_tx
    cons = sbce.qam.qam_constellation(4)

    def cn(*s):
        return (g.normal(size=s) + 1j * g.normal(size=s)) / np.sqrt(2)

    h = cn(2, L * n_rx)
    psi_d = np.exp(2j * np.pi * g.uniform(size=(2, T_d, P)))
    psi_p = np.exp(2j * np.pi * g.uniform(size=(2, T_p, P)))
    x_d, x_p = cons[g.integers(0, 4, (2, T_d, n_tx))], cons[g.integers(0, 4, (2, T_p, n_tx))]
    u_d = np.einsum("btp,bta->btpa", psi_d, x_d).reshape(2, T_d, L)
    u_p = np.einsum("btp,bta->btpa", psi_p, x_p).reshape(2, T_p, L)
    Hm = np.transpose(h.reshape(2, L, n_rx), (0, 2, 1))
    y_d, y_p = np.einsum("brl,btl->btr", Hm, u_d), np.einsum("brl,btl->btr", Hm, u_p)
    y_d[1] += np.sqrt(TRUE_VAR) * cn(T_d, n_rx)
    y_p[1] += np.sqrt(TRUE_VAR) * cn(T_p, n_rx)
    th0 = np.stack([np.linalg.lstsq(u_p[i], y_p[i], rcond=None)[0].reshape(-1) for i in range(2)])
    return dict(y_d=y_d, y_p=y_p, psi_d=psi_d, u_p=u_p, theta0=th0, cons=cons, n_tx=n_tx)


def test_floor_on_noiseless_data(sbce):
    b = _floor_batch(sbce)
    L = sbce._lib
    ref0 = _ref(b, 0, 6, 0.3, varn_min=1e-3)
    assert ref0["varn"] == 1e-3 and ref0["status"] == 64        # the restatement first
    r = sbce.em_batch_noise(*_args(b), b["cons"], 0.3, 6, b["theta0"], varn_min=1e-3)
    print("floor:", r["hist"], r["status"])
    assert r["varn"][0] == 1e-3 and np.all(r["hist"][0] == 1e-3)
    assert r["status"][0] & L.SBCE_STATUS_NOISE
    assert np.all(np.isfinite(r["theta"]))
    assert r["status"][1] == 0 and r["varn"][1] > 0.1
    assert np.isclose(r["varn"][1], _ref(b, 1, 6, 0.3, varn_min=1e-3)["varn"], rtol=1e-9, atol=0)


def test_early_stop_freezes_the_estimate(sbce):
    B = 4
    b = _batch(sbce, S22, B, seed=41)
    r = sbce.em_batch_noise(*_args(b), b["cons"], START, 5, b["theta0"], h_true=b["h"])
    free = sbce.em_batch_noise(*_args(b), b["cons"], START, 5, b["theta0"])
    print("early stop iters_done:", r["iters_done"])
    assert r["iters_done"].min() >= 2 and r["iters_done"].min() < 5
    for i in range(B):
        n = int(r["iters_done"][i])
        ref = orc.em_noise_ref(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, b["cons"], START,
                               5, b["theta0"][i], 2, h=b["h"][i])
        assert n == ref["iters_done"]
        assert r["varn"][i] == r["hist"][i, n - 1]
        assert np.all(r["hist"][i, n - 1:] == r["varn"][i])
        # up to its stop the trial is the free-running one: its last M-step was followed by its update
        assert np.array_equal(r["hist"][i, :n], free["hist"][i, :n])
        assert np.allclose(r["hist"][i], ref["hist"], rtol=1e-9, atol=0)
        assert rel(r["theta"][i], ref["theta"]) <= 1e-9


def test_em_batch_is_untouched_by_a_noise_run(sbce):
    b = _batch(sbce, S24, 4, seed=41)
    a0 = sbce.em_batch(*_args(b), b["cons"], START, 3, b["theta0"], h_true=b["h"])
    sbce.em_batch_noise(*_args(b), b["cons"], START, 3, b["theta0"], h_true=b["h"])
    a1 = sbce.em_batch(*_args(b), b["cons"], START, 3, b["theta0"], h_true=b["h"])
    for k in ("theta", "status", "iters_done"):
        assert np.array_equal(a0[k], a1[k]), k


def test_sweep_on_the_device(sbce):
    """noise_est_vs_snr through the real calls: the SNR axis in one call per curve equals the
    per-point calls bitwise, and its 'known' curve is nmse_vs_snr's exact-EM curve."""
    sw = sbce.sweeps
    kw = dict(SNR=(5, 15), T_d=20, T_p=8, N=4, n_rx=2, n_tx=2, itera=4, monte_iter=4, M=4, seed=3)
    snr, curves, ratio = sw.noise_est_vs_snr(varn_assumed=1.0, **kw)
    _, curves1, ratio1 = sw.noise_est_vs_snr(varn_assumed=1.0, batch_snr=False, **kw)
    for c in sw.NOISE_CURVES:
        assert np.array_equal(curves[c], curves1[c]), c
        assert np.all(np.isfinite(curves[c])) and curves[c].shape == (2,)
    assert np.array_equal(ratio, ratio1) and np.all(ratio > 0)
    _, ref = sw.nmse_vs_snr(modes=("soft",), **kw)
    assert np.array_equal(curves["known"], ref["soft"])
    print("sweep:", {c: curves[c] for c in curves}, ratio)


def test_noise_var_replays_in_a_graph(sbce):
    import torch
    L = sbce._lib
    lib = L.load()
    shape = SHAPES[5]
    n_tx, n_rx, P, T_p, T_d, M = shape
    B = 5
    b = _batch(sbce, shape, B, seed=61)
    ms, Ss = zip(*[orc.moments(b["theta0"][i], b["y_d"][i], b["psi_d"][i].T, b["cons"], START, n_tx,
                               "soft") for i in range(B)])
    mom = np.concatenate([np.stack(ms), np.stack(Ss).reshape(B, T_d, n_tx * n_tx)], axis=2)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex128)).cuda()
    Yd, Yp, Ps, Up, Th, Mo = (dev(b["y_d"]), dev(b["y_p"]), dev(b["psi_d"]), dev(b["u_p"]),
                              dev(b["theta0"]), dev(mom))
    dims = L.Dims(B, n_tx, n_rx, P, T_p, T_d, M, 0, START, 1.0)
    nb = ctypes.c_size_t(0)
    L.check(lib.sbce_noise_workspace_bytes(ctypes.byref(dims), ctypes.byref(nb)), "bytes")
    scratch = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    est = torch.zeros(B, dtype=torch.float64, device="cuda")
    ptrs = L.Ptrs(Yd.data_ptr(), Yp.data_ptr(), Ps.data_ptr(), Up.data_ptr(), None, Th.data_ptr(),
                  None, None, None, None, None, None, 0, None, None, None)
    opts = L.NoiseOpts(est.data_ptr(), None, scratch.data_ptr(), scratch.numel(), 1e-6, 0)

    def call():
        L.check(lib.sbce_noise_var(dims, ptrs, Mo.data_ptr(), opts,
                                   torch.cuda.current_stream().cuda_stream), "sbce_noise_var")

    call()
    torch.cuda.synchronize()
    eager = est.cpu().numpy().copy()
    assert np.all(eager > 0)
    est.zero_()
    scratch.zero_()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        est.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(est.cpu().numpy(), eager)
