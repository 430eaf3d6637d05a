"""GPU tier: the single-pass panel factor launches (csrc/chol.hip panel_factor_kernel) -- every
row tile read once, kept on chip through pre-update, TRSM-A, in-panel update and TRSM-B, and
written once; a tile's B half finishes from the registers when D_B^-1 is already published
(direct route) and after the launch's last barrier otherwise (deferred route).

Everything goes through sbce.mstep_batch; n_tx = 4 (8 in the last shape) keeps every shape on
the batched-panel path.  The bars are the ones test_gpu_em.py already holds for this solve."""
import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [
    # (n_tx, n_rx, N)  ->  L = (N+1) n_tx
    (4, 4, 8),       # L = 36: an odd panel 4 columns wide with no sub-panel B; a partial last row tile
    (4, 1, 12),      # L = 52: an odd panel with w_B = 4
    (4, 8, 16),      # L = 68: general back substitution; 8 right-hand sides through the fused y update
    (4, 4, 28),      # L = 116: 8 row tiles, two per tile wave, so both routes of a B half occur
    (4, 3, 43),      # L = 176: the last panel is odd with exactly 16 columns (w_B = 0 after a pre-update)
    (8, 4, 20),      # L = 168: n_tx = 8; the remainder panel is 8 columns wide
])
def test_onepass_factor_shapes(sbce, shape):
    """The generator and S = x x^H + 0.1 I of test_mfma_and_valu_cholesky_agree, 3 trials,
    T_p = 16, T_d = 60: against numpy.linalg.solve of the device's R, rhs < 1e-9, against the VALU
    Cholesky < 1e-9, against four real MFMAs per complex product < 1e-11."""
    n_tx, n_rx, N = shape
    b = sbce.signal_model.synthetic_batch(3, n_tx, n_rx, N, 16, 60, 4, 0.05, seed=4)
    x = b["x_d"]
    S = x[..., :, None] * np.conj(x[..., None, :]) + 0.1 * np.eye(n_tx)
    out = {}
    for impl, env in (("batched", {}), ("batched_c4", dict(SBCE_CPLX3="0")),
                      ("valu", dict(SBCE_CHOL_IMPL="valu"))):
        with sbce._lib.debug_env(**env):
            try:
                out[impl] = sbce.mstep_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], x,
                                             S, 0.05)
            except sbce._lib.SbceError as e:
                raise AssertionError(f"{impl}: {e}") from e
    th_m, R, rhs, st = out["batched"]
    assert R.shape[1] == (N + 1) * n_tx
    assert not st.any()
    for i in range(3):
        X = np.linalg.solve(R[i], rhs[i])                     # R X = B^H, theta = conj(X)
        ref = np.conj(X).reshape(-1)
        for impl in out:
            err = rel(out[impl][0][i], ref)
            print(f"L={R.shape[1]} trial {i} {impl}: vs numpy {err:.3e}")
            assert err < 1e-9, impl
    e4, ev = rel(th_m, out["batched_c4"][0]), rel(th_m, out["valu"][0])
    print(f"L={R.shape[1]}: vs four-MFMA {e4:.3e}, vs VALU {ev:.3e}")
    assert e4 < 1e-11
    assert ev < 1e-9


def test_route_independence_bitwise(sbce):
    """L = 116: trial 0's theta and status are bitwise the same solved alone, in a batch of 3, in
    a batch of 520 (several workgroups per CU, so the direct / deferred choice falls differently),
    in two repeated calls, and in a 0x00 and a 0xFF workspace."""
    n_tx, n_rx, N = 4, 4, 28
    b = sbce.signal_model.synthetic_batch(520, n_tx, n_rx, N, 16, 60, 4, 0.05, seed=4)
    x = b["x_d"]
    S = x[..., :, None] * np.conj(x[..., None, :]) + 0.1 * np.eye(n_tx)

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


def test_rank_deficient_R_at_116(sbce):
    """L = 116, S = x x^H unregularised (T_p + T_d = 76 < L): the properties of
    test_chol_on_rank_deficient_R_is_finite_flagged_and_minnorm_on_range -- theta finite, every
    trial flagged NONHPD, bitwise the same in a 0x00 and a 0xFF workspace, residual and range-space
    part at 1e-10.  The CPU restatement of the policy (oracle.mstep_chol_policy) meets the bar on
    this input (residual <= 3e-14, range part <= 1e-13 at seed 11) and is asserted alongside."""
    from oracle.em_reduced import mstep_build, mstep_chol_policy, mstep_lstsq, range_part
    n_tx, n_rx, N, T_p, T_d, M = 4, 4, 28, 16, 60, 16
    varn = float(sbce.signal_model.snr_to_varn(20.0))
    b = sbce.signal_model.synthetic_batch(2, n_tx, n_rx, N, T_p, T_d, M, varn, seed=11)
    x = b["x_d"]
    S = x[..., :, None] * np.conj(x[..., None, :])
    args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], x, S, varn)
    outs = [sbce.mstep_batch(*args, solve="chol", ws_fill=f) for f in (0x00, 0xFF)]
    th, R, rhs, st = outs[0]
    assert np.isfinite(th).all()
    assert np.array_equal(th.view(np.uint64), outs[1][0].view(np.uint64))
    assert np.array_equal(st, outs[1][3])
    assert (st & sbce._lib.SBCE_STATUS_NONHPD).all()
    for i in range(2):
        R0, rhs0 = mstep_build(b["u_p"][i], b["y_p"][i], b["psi_d"][i].T, b["y_d"][i], x[i], S[i])
        lo = np.tril_indices(R0.shape[0])
        assert rel(R[i][lo], R0[lo]) < 1e-12
        th_ls, rank = mstep_lstsq(R0, rhs0)
        assert rank <= T_p + T_d < R0.shape[0] == 116
        X = np.conj(th[i]).reshape(R0.shape[0], n_rx)
        res = np.abs(R0 @ X - rhs0).max() / np.abs(rhs0).max()
        rng = rel(range_part(R0, th[i], n_rx), th_ls)
        print(f"trial {i}: residual {res:.3e}, range part {rng:.3e}")
        assert res < 1e-10
        assert rng < 1e-10
        th_cpu, _ = mstep_chol_policy(R0, rhs0)
        assert rel(range_part(R0, th_cpu, n_rx), th_ls) < 1e-10
