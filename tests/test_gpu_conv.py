"""GPU tier of the log-likelihood readout and the truth-free convergence stop: sbce_loglik
(csrc/loglik.hip) against the NumPy restatement at every kernel path, its batch independence and
graph capture, and sbce_em_conv against the restated loop: stop iterations, frozen trials, the
unchanged chain when no stop can happen, the noise estimate beside the stop, the ll history and
rule, the other E-step modes and the sweep."""
import ctypes

import numpy as np
import pytest

from conftest import rel
import conv_oracle as orc

pytestmark = pytest.mark.gpu

# (n_tx, n_rx, P, T_p, T_d, M): a single stream; two streams at 4- and 16-QAM; odd n_rx and ragged
# T_d; more than one theta tile (P = 33); n_rx = 8 (the 8-row instantiation); J = 4096 (four
# symbols per workgroup, 64 row blocks); J = 65536 at six symbols (two workgroups, 4096 row blocks)
SHAPES = [(1, 2, 8, 8, 30, 16), (2, 2, 8, 16, 40, 4), (2, 4, 8, 16, 40, 16), (3, 5, 5, 12, 33, 4),
          (4, 4, 33, 16, 64, 4), (2, 8, 3, 8, 20, 4), (2, 2, 16, 8, 20, 64), (4, 4, 4, 8, 6, 16)]
S22, S24, S44W, S88 = SHAPES[1], SHAPES[2], SHAPES[4], (8, 8, 3, 16, 24, 4)
VARNS = (0.01, 0.3, 30.0)
TRUE_VAR = 0.3
_cache = {}


def _batch(sbce, shape, B, seed, varn=TRUE_VAR):
    key = (shape, B, seed, varn)
    if key not in _cache:
        n_tx, n_rx, P, T_p, T_d, M = shape
        _cache[key] = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, varn,
                                                        seed=seed, pinv="scipy")
    return _cache[key]


def _args(b, sl=slice(None)):
    return b["y_d"][sl], b["y_p"][sl], b["psi_d"][sl], b["u_p"][sl]


def _trial(b, i):
    return b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, b["cons"]


def _ref(b, i, start, itera, **kw):
    """em_conv_ref of trial i, computed once per (batch, arguments)."""
    key = ("ref", id(b), i, start, itera, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = orc.em_conv_ref(*_trial(b, i), start, itera, b["theta0"][i], b["n_tx"], **kw)
    return _cache[key]


def _away(refs, tol=True, ll=False):
    """The restatement's decisions all lie outside [0.95, 1.05] of their thresholds (a condition
    on the inputs: pick another seed on the CPU if a later change breaks it)."""
    vals = [d for r in refs for d in (r["delta"] if tol else [])]
    vals += [d for r in refs for d in (r["dll"] if ll else [])]
    return all(not 0.95 <= d <= 1.05 for d in vals)


# ------------------------------------------------------------------ sbce_loglik
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loglik_matches_restatement(sbce, shape):
    """|ll - ref| <= 1e-12 A and |ll_sym - ref| <= 1e-12 A_t at a hardened (d/s2 ~ 1e6), a moderate
    and a flat posterior: every residual entry stands behind at most L + 2 rounded products."""
    n_tx = shape[0]
    B = 3
    b = _batch(sbce, shape, B, seed=31)
    for v in VARNS:
        ll, sym = sbce.loglik_batch(*_args(b), b["cons"], b["theta0"], v, n_tx, per_symbol=True)
        only = sbce.loglik_batch(*_args(b), b["cons"], b["theta0"], v, n_tx)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(sym))
        assert np.array_equal(only, ll)              # the per-symbol output does not change ll
        worst = worst_t = 0.0
        for i in range(B):
            Y_d, Y_p, U_p, Psi, cons = _trial(b, i)
            A, A_t = orc.error_scale(Y_d, Y_p, U_p, Psi, cons, b["theta0"][i], v, n_tx)
            ref = orc.loglik_ref(Y_d, Y_p, U_p, Psi, cons, b["theta0"][i], v, n_tx)
            ref_t = orc.loglik_sym_ref(Y_d, Psi, cons, b["theta0"][i], v, n_tx)
            worst = max(worst, abs(ll[i] - ref) / (1e-12 * A))
            worst_t = max(worst_t, (np.abs(sym[i] - ref_t) / (1e-12 * A_t)).max())
        print(f"loglik {shape} varn {v}: |d ll| / bound = {worst:.3e}, per symbol {worst_t:.3e}")
        assert worst <= 1.0 and worst_t <= 1.0


def test_loglik_without_pilots(sbce):
    b = _batch(sbce, S22, 2, seed=31)
    y_p, u_p = b["y_p"][:, :0], b["u_p"][:, :0]
    ll, sym = sbce.loglik_batch(b["y_d"], y_p, b["psi_d"], u_p, b["cons"], b["theta0"], 0.3, 2,
                                per_symbol=True)
    full, sym_full = sbce.loglik_batch(*_args(b), b["cons"], b["theta0"], 0.3, 2, per_symbol=True)
    assert np.array_equal(sym, sym_full) and np.all(ll != full)
    for i in range(2):
        assert abs(ll[i] - sym[i].sum()) <= 1e-13 * np.abs(sym[i]).sum()


def test_loglik_trial_is_bitwise_independent_of_the_batch(sbce):
    b = _batch(sbce, S44W, 37, seed=51)
    vt = np.linspace(0.05, 2.0, 37)
    big, big_sym = sbce.loglik_batch(*_args(b), b["cons"], b["theta0"], 0.3, 4, per_symbol=True)
    per = sbce.loglik_batch(*_args(b), b["cons"], b["theta0"], vt, 4)
    for i in (0, 18, 36):
        sl = slice(i, i + 1)
        one, one_sym = sbce.loglik_batch(*_args(b, sl), b["cons"], b["theta0"][sl], 0.3, 4,
                                         per_symbol=True)
        assert np.array_equal(big[sl], one) and np.array_equal(big_sym[sl], one_sym), i
        sc = sbce.loglik_batch(*_args(b, sl), b["cons"], b["theta0"][sl], float(vt[i]), 4)
        assert np.array_equal(per[sl], sc), i
    assert not np.array_equal(per, big)


def test_loglik_replays_in_a_graph(sbce):
    import torch
    L = sbce._lib
    lib = L.load()
    n_tx, n_rx, P, T_p, T_d, M = S44W
    B = 5
    b = _batch(sbce, S44W, B, seed=61)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex128)).cuda()
    Yd, Yp, Ps, Up, Cs, Th = (dev(b["y_d"]), dev(b["y_p"]), dev(b["psi_d"]), dev(b["u_p"]),
                              dev(b["cons"]), dev(b["theta0"]))
    dims = L.Dims(B, n_tx, n_rx, P, T_p, T_d, M, 0, 0.3, 1.0)
    nb = ctypes.c_size_t(0)
    L.check(lib.sbce_loglik_workspace_bytes(ctypes.byref(dims), ctypes.byref(nb)), "bytes")
    scratch = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    ll = torch.zeros(B, dtype=torch.float64, device="cuda")
    sym = torch.zeros((B, T_d), dtype=torch.float64, device="cuda")
    ptrs = L.Ptrs(Yd.data_ptr(), Yp.data_ptr(), Ps.data_ptr(), Up.data_ptr(), Cs.data_ptr(),
                  Th.data_ptr(), None, None, None, None, None, None, 0, None, None, None)

    def call():
        L.check(lib.sbce_loglik(dims, ptrs, ll.data_ptr(), sym.data_ptr(), scratch.data_ptr(),
                                scratch.numel(), torch.cuda.current_stream().cuda_stream),
                "sbce_loglik")

    call()
    torch.cuda.synchronize()
    eager, eager_sym = ll.cpu().numpy().copy(), sym.cpu().numpy().copy()
    assert np.all(np.isfinite(eager)) and np.all(eager != 0)
    assert np.array_equal(Th.cpu().numpy(), b["theta0"])         # theta is read, never written
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        ll.zero_()
        sym.zero_()
        scratch.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ll.cpu().numpy(), eager)
        assert np.array_equal(sym.cpu().numpy(), eager_sym)


# ------------------------------------------------------------------ sbce_em_conv
MAXIT = 16


def _stop_run(sbce):
    if "stop" not in _cache:
        b = _batch(sbce, S22, 4, seed=21)
        _cache["stop"] = (b, sbce.em_batch_conv(*_args(b), b["cons"], TRUE_VAR, MAXIT, b["theta0"]))
    return _cache["stop"]


def test_em_conv_matches_restated_loop(sbce):
    """tol_theta 1e-6, min_iters 2, at most 16 iterations: the stop iteration and the CONVERGED
    bit equal the restatement's, theta at the driver bar 1e-9, dtheta_hist at 4e-9 absolute (two
    theta errors over ||theta||)."""
    L = sbce._lib
    b, r = _stop_run(sbce)
    refs = [_ref(b, i, TRUE_VAR, MAXIT) for i in range(4)]
    assert len({q["iters_done"] for q in refs}) >= 3, [q["iters_done"] for q in refs]
    assert _away(refs)
    print("em_conv iters_done", r["iters_done"], "status", r["status"])
    for i, q in enumerate(refs):
        assert r["iters_done"][i] == q["iters_done"], i
        assert (r["status"][i] & L.SBCE_STATUS_CONVERGED) == (q["status"] & orc.STATUS_CONVERGED)
        assert rel(r["theta"][i], q["theta"]) <= 1e-9
        assert np.abs(r["dtheta_hist"][i] - q["dtheta_hist"]).max() <= 4e-9
    assert r["ll_hist"] is None and r["hist"] is None
    assert np.array_equal(r["varn"], np.full(4, TRUE_VAR))


def test_a_stopped_trial_is_frozen(sbce):
    """A trial that stopped after k iterations holds bitwise the theta of a one-trial call with
    k iterations and no stop possible, and its history stays at its last value."""
    b, r = _stop_run(sbce)
    stopped = [i for i in range(4) if r["iters_done"][i] < MAXIT]
    assert stopped
    for i in stopped:
        k = int(r["iters_done"][i])
        sl = slice(i, i + 1)
        one = sbce.em_batch_conv(*_args(b, sl), b["cons"], TRUE_VAR, k, b["theta0"][sl], min_iters=k)
        assert np.array_equal(one["theta"], r["theta"][sl]), i
        assert np.array_equal(one["dtheta_hist"][0], r["dtheta_hist"][i, :k])
        assert np.all(r["dtheta_hist"][i, k - 1:] == r["dtheta_hist"][i, k - 1])


def test_chain_is_unchanged_when_no_stop_can_happen(sbce):
    b = _batch(sbce, S22, 4, seed=21)
    it = 5
    plain = sbce.em_batch(*_args(b), b["cons"], TRUE_VAR, it, b["theta0"])
    conv = sbce.em_batch_conv(*_args(b), b["cons"], TRUE_VAR, it, b["theta0"], min_iters=it)
    assert np.array_equal(conv["theta"], plain["theta"])
    assert np.array_equal(conv["iters_done"], np.full(4, it))
    noise = sbce.em_batch_noise(*_args(b), b["cons"], 1.0, it, b["theta0"])
    convn = sbce.em_batch_conv(*_args(b), b["cons"], 1.0, it, b["theta0"], min_iters=it,
                               estimate_noise=True)
    assert np.array_equal(convn["theta"], noise["theta"])
    assert np.array_equal(convn["varn"], noise["varn"])
    assert np.array_equal(convn["hist"], noise["hist"])
    # and a conv run leaves the plain chain as it was
    again = sbce.em_batch(*_args(b), b["cons"], TRUE_VAR, it, b["theta0"])
    assert np.array_equal(again["theta"], plain["theta"])


def test_noise_estimate_and_stop_together(sbce):
    b = _batch(sbce, S22, 4, seed=21)
    r = sbce.em_batch_conv(*_args(b), b["cons"], 1.0, MAXIT, b["theta0"], estimate_noise=True)
    refs = [_ref(b, i, 1.0, MAXIT, estimate_noise=True) for i in range(4)]
    assert _away(refs)
    print("em_conv + noise iters_done", r["iters_done"], "varn", r["varn"])
    for i, q in enumerate(refs):
        k = q["iters_done"]
        assert r["iters_done"][i] == k, i
        assert rel(r["theta"][i], q["theta"]) <= 1e-9
        assert abs(r["varn"][i] / q["varn"] - 1) <= 1e-9
        assert np.allclose(r["hist"][i], q["hist"], rtol=1e-9, atol=0)
        assert np.all(r["hist"][i, k - 1:] == r["varn"][i])
    assert np.array_equal(r["sigma2"], r["varn"] ** 2)


def test_ll_hist_and_the_ll_rule(sbce):
    b = _batch(sbce, S22, 4, seed=21)
    r = sbce.em_batch_conv(*_args(b), b["cons"], TRUE_VAR, MAXIT, b["theta0"], loglik=True)
    refs = [_ref(b, i, TRUE_VAR, MAXIT, loglik=True) for i in range(4)]
    for i, q in enumerate(refs):
        k = q["iters_done"]
        assert r["iters_done"][i] == k
        for l in range(MAXIT):
            th, v = q["trace"][min(l, k - 1)]
            A, _ = orc.error_scale(*_trial(b, i), th, v, 2)
            assert abs(r["ll_hist"][i, l] - q["ll_hist"][l]) <= 1e-9 * A, (i, l)
        d = np.diff(r["ll_hist"][i])
        assert np.all(d >= -1e-9 * np.abs(r["ll_hist"][i, 1:])), (i, d)
    # the log-likelihood costs nothing in theta: the run without it gives the same bits
    _, plain = _stop_run(sbce)
    assert np.array_equal(plain["theta"], r["theta"])
    # the ll rule
    s = sbce.em_batch_conv(*_args(b), b["cons"], TRUE_VAR, MAXIT, b["theta0"], loglik=True,
                           tol_ll=1e-9)
    refs = [_ref(b, i, TRUE_VAR, MAXIT, loglik=True, tol_ll=1e-9) for i in range(4)]
    assert _away(refs, ll=True)
    print("ll rule iters_done", s["iters_done"], [q["iters_done"] for q in refs])
    for i, q in enumerate(refs):
        assert s["iters_done"][i] == q["iters_done"], i
        assert rel(s["theta"][i], q["theta"]) <= 1e-9
    # some trial is stopped by the ll rule before the theta rule would
    assert any(q["iters_done"] < p["iters_done"]
               for q, p in zip(refs, [_ref(b, i, TRUE_VAR, MAXIT) for i in range(4)]))


# hard: converges to an exact fixed point (the decisions stop changing).  zf and pm_soft do not
# contract on these data (the restatement's relative step stays near 1), so their rule is set at
# tol_theta = 3 with min_iters = 3: every trial stops after three iterations and the two masked
# iterations that follow must leave theta alone.
MODE_CASES = [(S24, "hard", 0, 21, TRUE_VAR, 12, dict()),
              (S22, "zf", 0, 41, 1.0, 5, dict(tol_theta=3.0, min_iters=3)),
              (S88, "pm_soft", 1, 41, 1.0, 5, dict(tol_theta=3.0, min_iters=3))]


@pytest.mark.parametrize("shape,mode,pr,seed,start,iters,kw", MODE_CASES,
                         ids=[c[1] for c in MODE_CASES])
def test_other_estep_modes_theta_rule(sbce, shape, mode, pr, seed, start, iters, kw):
    B = 3
    b = _batch(sbce, shape, B, seed=seed)
    refs = [_ref(b, i, start, iters, mode=mode, partition_r=pr, **kw) for i in range(B)]
    assert _away(refs)
    assert all(q["iters_done"] < iters for q in refs), [q["iters_done"] for q in refs]
    r = sbce.em_batch_conv(*_args(b), b["cons"], start, iters, b["theta0"], mode=mode,
                           partition_r=pr, **kw)
    print(f"em_conv {mode}: iters_done {r['iters_done']} status {r['status']}")
    for i, q in enumerate(refs):
        assert r["iters_done"][i] == q["iters_done"], i
        assert r["status"][i] & sbce._lib.SBCE_STATUS_CONVERGED
        assert rel(r["theta"][i], q["theta"]) <= 1e-9


def test_loglik_beyond_its_limits_is_unsupported(sbce):
    b = _batch(sbce, S88, 3, seed=41)
    with pytest.raises(sbce.SbceError, match=r"\(-2\)"):
        sbce.em_batch_conv(*_args(b), b["cons"], 1.0, 3, b["theta0"], mode="pm_soft", partition_r=1,
                           loglik=True)


def test_sweep_on_the_device(sbce):
    sw = sbce.sweeps
    kw = dict(SNR=(5, 15), T_d=20, T_p=8, N=4, n_rx=2, n_tx=2, itera=8, monte_iter=8, M=4, seed=3)
    snr, nmse, its = sw.convergence_vs_snr(**kw)
    print("convergence sweep:", nmse, its)
    assert list(snr) == [5, 15] and tuple(nmse) == tuple(its) == sw.CONV_ARMS
    for arm in sw.CONV_ARMS:
        assert nmse[arm].shape == (2,) and np.all(np.isfinite(nmse[arm]))
        assert np.all(its[arm] >= 1) and np.all(its[arm] <= 8)
    assert np.all(its["fixed"] == 8) and np.all(its["stop"] <= 8)
    _, ref = sw.nmse_vs_snr(modes=("soft",), **kw)
    assert np.array_equal(nmse["fixed"], ref["soft"])
    _, nmse1, its1 = sw.convergence_vs_snr(batch_snr=False, **kw)
    for arm in sw.CONV_ARMS:
        assert np.array_equal(nmse[arm], nmse1[arm]) and np.array_equal(its[arm], its1[arm])
