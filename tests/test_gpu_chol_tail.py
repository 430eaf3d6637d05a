"""GPU tier: the remainder fold of the batched panel Cholesky (csrc/chol.hip tail_fold) -- a last
panel of at most four columns gets no update and no factor launch; backsub4_kernel factors it at
its head from the factor rows it loads anyway.

Everything goes through sbce.mstep_batch / em_batch / EMEngine; n_tx = 4 keeps L <= 64 on the
batched-panel path.  The bars are the ones test_gpu_em.py and test_gpu_chol_onepass.py hold for
this solve; SBCE_BACKSUB=1 (general back substitution) keeps the unfolded schedule and is the
cross-check."""
import ctypes

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu


def _regularised(sbce, nb, n_tx, n_rx, N):
    """The generator and S = x x^H + 0.1 I of test_onepass_factor_shapes (T_p = 16, T_d = 60, 4-QAM,
    seed 4).  R has rank <= n_tx T_d + T_p, which is 256 at T_d = 60: at L = 260 that R is singular
    (numpy rank 256, cond 9e15; oracle.mstep_chol_policy drops the four remainder pivots as the
    device does), so L = 260 takes cfg1's T_d = 256, where cond(R) = 1.2e2 as at the other
    shapes."""
    T_d = 256 if (N + 1) * n_tx > 4 * 60 + 16 else 60
    b = sbce.signal_model.synthetic_batch(nb, n_tx, n_rx, N, 16, T_d, 4, 0.05, seed=4)
    x = b["x_d"]
    S = x[..., :, None] * np.conj(x[..., None, :]) + 0.1 * np.eye(n_tx)
    return b, x, S


@pytest.mark.parametrize("shape", [
    # (n_tx, n_rx, N)  ->  L = (N+1) n_tx
    (4, 4, 8),       # L = 36: odd last panel, NR 4
    (4, 1, 16),      # L = 68: even last panel, NR 1
    (4, 3, 24),      # L = 100: odd last panel, NR 3
    (1, 2, 64),      # L = 65: w = 1
    (4, 2, 64),      # L = 260: cfg1's panel layout
    (3, 4, 22),      # L = 69: w = 5, not folded
    (4, 8, 16),      # L = 68: NR 8, not folded
])
def test_folded_and_unfolded_shapes(sbce, shape):
    """3 trials, T_p = 16, T_d = 60 (256 at L = 260, see _regularised): against numpy.linalg.solve
    of the device's R, rhs < 1e-9, against the VALU Cholesky < 1e-9, against four real MFMAs per
    complex product < 1e-11, against the unfolded schedule (SBCE_BACKSUB=1) < 1e-12; status 0."""
    n_tx, n_rx, N = shape
    b, x, S = _regularised(sbce, 3, n_tx, n_rx, N)
    out = {}
    for impl, env in (("batched", {}), ("batched_c4", dict(SBCE_CPLX3="0")),
                      ("valu", dict(SBCE_CHOL_IMPL="valu")), ("general", dict(SBCE_BACKSUB="1"))):
        with sbce._lib.debug_env(**env):
            try:
                out[impl] = sbce.mstep_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], x,
                                             S, 0.05)
            except sbce._lib.SbceError as e:
                raise AssertionError(f"{impl}: {e}") from e
    th_m, R, rhs, st = out["batched"]
    L = R.shape[1]
    assert L == (N + 1) * n_tx
    assert not st.any()
    for i in range(3):
        X = np.linalg.solve(R[i], rhs[i])                     # R X = B^H, theta = conj(X)
        ref = np.conj(X).reshape(-1)
        e_np = rel(th_m[i], ref)
        e_v = rel(th_m[i], out["valu"][0][i])
        e_4 = rel(th_m[i], out["batched_c4"][0][i])
        e_g = rel(th_m[i], out["general"][0][i])
        print(f"L={L} trial {i}: vs numpy {e_np:.3e}, VALU {e_v:.3e}, four-MFMA {e_4:.3e}, "
              f"unfolded {e_g:.3e}")
        assert e_np < 1e-9
        assert e_v < 1e-9
        assert e_4 < 1e-11
        assert e_g < 1e-12


def _launch_counts(sbce, n_tx, n_rx, N):
    """(update, factor, back-substitution) launches of one M-step (sbce_debug_chol_timing)."""
    import torch
    b, x, S = _regularised(sbce, 3, n_tx, n_rx, N)
    fn = sbce._lib.load().sbce_debug_chol_timing
    fn.restype = ctypes.c_int
    out6 = (ctypes.c_double * 6)()
    torch.cuda.synchronize()
    assert fn(1, None) == 0
    try:
        sbce.mstep_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], x, S, 0.05)
    finally:
        torch.cuda.synchronize()
        rc = fn(0, out6)
    assert rc == 0
    return tuple(int(round(v)) for v in out6[3:6])


@pytest.mark.parametrize("shape, counts", [
    ((4, 2, 64), (3, 8, 1)),     # L = 260: panel 8 (even, 4 columns) folded
    ((4, 3, 24), (1, 3, 1)),     # L = 100: panel 3 (odd, 4 columns) folded
    ((3, 4, 22), (1, 3, 1)),     # L = 69: w = 5, unchanged
])
def test_launch_counts(sbce, shape, counts):
    assert _launch_counts(sbce, *shape) == counts


def test_fold_independence_bitwise(sbce):
    """L = 68: trial 0's theta and status are bitwise the same solved alone, in a batch of 3, in a
    batch of 520, in two repeated calls, and in a 0x00 and a 0xFF workspace."""
    b, x, S = _regularised(sbce, 520, 4, 1, 16)

    def run(nb, **kw):
        th, _, _, st = sbce.mstep_batch(b["y_d"][:nb], b["y_p"][:nb], b["psi_d"][:nb], b["u_p"][:nb],
                                        b["cons"], x[:nb], S[:nb], 0.05, **kw)
        return np.ascontiguousarray(th[0]).view(np.uint64).copy(), int(st[0])

    ref = run(1)
    assert np.isfinite(ref[0].view(np.float64)).all() and ref[1] == 0
    for what, got in (("batch of 3", run(3)), ("batch of 520", run(520)), ("repeat", run(520)),
                      ("repeat alone", run(1)), ("ws 0x00", run(3, ws_fill=0x00)),
                      ("ws 0xFF", run(3, ws_fill=0xFF)), ("ws 0xFF, 520", run(520, ws_fill=0xFF))):
        assert np.array_equal(got[0], ref[0]), what
        assert got[1] == ref[1], what


@pytest.mark.parametrize("shape, rank_np", [
    ((4, 4, 8, 16, 12), 28),       # L = 36
    ((4, 4, 16, 16, 40), 56),      # L = 68
    ((4, 2, 64, 16, 200), 216),    # L = 260
])
def test_dropped_pivots_inside_the_remainder(sbce, shape, rank_np):
    """S = x x^H unregularised, 16-QAM, 20 dB, seed 11 (T_p + T_d < L, so pivots of the folded
    block are dropped): the properties of test_rank_deficient_R_at_116 -- theta finite, every trial
    flagged NONHPD, bitwise the same in a 0x00 and a 0xFF workspace, residual and range-space part
    at 1e-10 against lstsq.  The CPU restatement of the policy (oracle.mstep_chol_policy) meets
    the bar on these inputs (residual <= 3e-14, range part <= 3e-13) and is asserted alongside."""
    from oracle.em_reduced import mstep_build, mstep_chol_policy, mstep_lstsq, range_part
    n_tx, n_rx, N, T_p, T_d = shape
    varn = float(sbce.signal_model.snr_to_varn(20.0))
    b = sbce.signal_model.synthetic_batch(2, n_tx, n_rx, N, T_p, T_d, 16, varn, seed=11)
    x = b["x_d"]
    S = x[..., :, None] * np.conj(x[..., None, :])
    args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], x, S, varn)
    outs = [sbce.mstep_batch(*args, solve="chol", ws_fill=f) for f in (0x00, 0xFF)]
    th, R, rhs, st = outs[0]
    L = (N + 1) * n_tx
    assert np.isfinite(th).all()
    assert np.array_equal(th.view(np.uint64), outs[1][0].view(np.uint64))
    assert np.array_equal(st, outs[1][3])
    assert (st & sbce._lib.SBCE_STATUS_NONHPD).all()
    for i in range(2):
        R0, rhs0 = mstep_build(b["u_p"][i], b["y_p"][i], b["psi_d"][i].T, b["y_d"][i], x[i], S[i])
        lo = np.tril_indices(L)
        assert rel(R[i][lo], R0[lo]) < 1e-12
        th_ls, rank = mstep_lstsq(R0, rhs0)
        assert rank == rank_np < L
        X = np.conj(th[i]).reshape(L, n_rx)
        res = np.abs(R0 @ X - rhs0).max() / np.abs(rhs0).max()
        rng = rel(range_part(R0, th[i], n_rx), th_ls)
        th_cpu, _ = mstep_chol_policy(R0, rhs0)
        Xc = np.conj(th_cpu).reshape(L, n_rx)
        res_cpu = np.abs(R0 @ Xc - rhs0).max() / np.abs(rhs0).max()
        rng_cpu = rel(range_part(R0, th_cpu, n_rx), th_ls)
        print(f"L={L} trial {i}: residual {res:.3e}, range part {rng:.3e} "
              f"(CPU policy {res_cpu:.3e}, {rng_cpu:.3e})")
        assert res < 1e-10
        assert rng < 1e-10
        assert res_cpu < 1e-10
        assert rng_cpu < 1e-10


def test_em_loop_repeats_bitwise_on_the_folded_schedule(sbce):
    """(4,4,8), T_p = 16, T_d = 40, 4-QAM, varn 0.05, 3 trials, exact soft E-step, 4 iterations
    (L = 36: the sphere E-step with its work lists and counters, the folded batched-panel M-step):
    against oracle.em_reduced at 1e-9; a second run on the same engine and workspace, and a run in
    a 0xFF-filled workspace, are bitwise equal to the first.  (Written for the list counters
    zeroed by the M-step's last launch, which was measured and not kept -- DESIGN section 3.5; the
    checks hold for the per-E-step memset as well and stay.)"""
    import torch
    from oracle.em_reduced import em_reduced
    varn = 0.05
    b = sbce.signal_model.synthetic_batch(3, 4, 4, 8, 16, 40, 4, varn, seed=4)
    aps = sbce.qam.all_possible_symbols(b["cons"], 4)
    r = sbce.em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], varn, 4, b["theta0"])
    assert not r["status"].any()
    for i in range(3):
        ref = em_reduced(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, aps, varn, 4,
                         b["theta0"][i])
        err = rel(r["theta"][i], ref)
        print(f"trial {i}: vs oracle {err:.3e}")
        assert err < 1e-9
    eng = sbce.EMEngine(b, varn)
    eng.ws_all.fill_(0x00)
    first = eng.run(4).clone()
    st_first = eng.status.clone()
    second = eng.run(4).clone()
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), r["theta"])
    assert torch.equal(first, second) and torch.equal(st_first, eng.status)
    eng_ff = sbce.EMEngine(b, varn)
    eng_ff.ws_all.fill_(0xFF)
    third = eng_ff.run(4).clone()
    torch.cuda.synchronize()
    assert torch.equal(first, third) and torch.equal(st_first, eng_ff.status)
