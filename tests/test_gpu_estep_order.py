"""The V16 soft sweep's best-first order (csrc/estep_sweep.hip: column tiles by ascending
column-tile bound, the row blocks of a tile by ascending block minimum of the row-tile bound;
SBCE_ESTEP_ORDER=0 in the A/B build is the natural order 0, 1, 2, ...).

The order decides only when a tile group is met: the groups that are swept hold every hypothesis
the posterior keeps under either order, so the soft moments agree to the project's bar for two
writers of one posterior, 1e-11 max|c|^2 (the sums change order, not content), and to the
oracle's enumeration of all 65,536 hypotheses.  The hard decision keeps the natural order and is
bitwise unchanged.  Equal bounds keep the natural order (bitwise equal results), the E-step stays
deterministic, and the counters (SBCE_ESTEP_COUNT=1) show fewer FP64 groups, in line with the CPU
restatement tools/e0_group_bounds.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle.em_reduced import estep_moments

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import e0_group_bounds as gb  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-11          # times max|c|^2: two writers of the same posterior


def _near_true(b):
    return b["h"] + 0.05 * b["theta0"] / np.abs(b["theta0"]).max()


def _estep(sbce, b, th, varn, mode, **env):
    with sbce._lib.debug_env(**env):
        return sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], th, varn, 4, mode)


def _batch(sbce, n_rx, snr):
    varn = float(sbce.signal_model.snr_to_varn(snr))
    return varn, sbce.signal_model.synthetic_batch(4, 4, n_rx, 8, 16, 32, 16, varn, seed=70 + snr + n_rx)


@pytest.mark.parametrize("snr", [30, 20, 10, 0, -5])
@pytest.mark.parametrize("n_rx", [3, 4, 8])
def test_same_posterior(sbce, n_rx, snr):
    varn, b = _batch(sbce, n_rx, snr)
    scale = np.abs(b["cons"]).max() ** 2
    for name, th in (("theta0", b["theta0"]), ("near", _near_true(b))):
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="0", SBCE_ESTEP_SPHERE=sph)
            dm, dS = np.abs(m1 - m0).max(), np.abs(S1 - S0).max()
            print(f"n_rx {n_rx} snr {snr} {name} sphere {sph}: |dm| {dm:.2e} |dS| {dS:.2e} (bar {BAR * scale:.2e})")
            assert np.isfinite(m1).all() and np.isfinite(S1).all()
            assert dm < BAR * scale and dS < BAR * scale, (n_rx, snr, name, sph, dm, dS)


def test_against_the_oracle_enumeration(sbce):
    """theta_0, 20 dB, n_rx = 4: the ordered sweep against all 65,536 hypotheses per symbol."""
    varn, b = _batch(sbce, 4, 20)
    scale = np.abs(b["cons"]).max() ** 2
    aps = sbce.qam.all_possible_symbols(b["cons"], 4)
    ref = [estep_moments(b["theta0"][i], b["y_d"][i], b["psi_d"][i].T, aps, varn)[:2] for i in range(4)]
    for sph in ("1", "0"):
        m, S = _estep(sbce, b, b["theta0"], varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
        for i, (m0, S0) in enumerate(ref):
            dm, dS = np.abs(m[i] - m0).max(), np.abs(S[i] - S0).max()
            print(f"sphere {sph} trial {i}: |dm| {dm:.2e} |dS| {dS:.2e} (bar {BAR * scale:.2e})")
            assert dm < BAR * scale and dS < BAR * scale, (sph, i, dm, dS)


@pytest.mark.parametrize("snr", [30, 20, 10, 0, -5])
@pytest.mark.parametrize("n_rx", [3, 4, 8])
def test_hard_mode_is_untouched(sbce, n_rx, snr):
    varn, b = _batch(sbce, n_rx, snr)
    for th in (b["theta0"], _near_true(b)):
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "hard", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "hard", SBCE_ESTEP_ORDER="0", SBCE_ESTEP_SPHERE=sph)
            assert np.array_equal(m1, m0) and np.array_equal(S1, S0), (n_rx, snr, sph)


def _zeroed(b, n_rx, streams):
    th = b["theta0"].reshape(b["theta0"].shape[0], -1, 4, n_rx).copy()
    for q in streams:
        th[:, :, q, :] = 0.0
    return th.reshape(b["theta0"].shape)


def _same_bits(sbce, b, th, varn):
    out = True
    for sph in ("1", "0"):
        m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
        m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="0", SBCE_ESTEP_SPHERE=sph)
        out = out and np.array_equal(m1, m0) and np.array_equal(S1, S0)
    return out


def test_ties_keep_the_natural_order_n_rx_2(sbce):
    """n_rx = 2: both projectors are 0, every column-tile and row-tile bound is 0, and the ordered
    sweep is the natural one, bit for bit."""
    for snr in (20, 0):
        varn, b = _batch(sbce, 2, snr)
        for th in (b["theta0"], _near_true(b)):
            assert _same_bits(sbce, b, th, varn), snr


def test_ties_keep_the_natural_order_zero_columns(sbce):
    """h_0 = h_2 = 0 (n_rx = 4): x_2 = cons[kt] and x_0 drop out of both bounds, so the 16
    column-tile bounds are bit-equal and so are the 16 row-tile bounds of every tile: the ordered
    sweep is the natural one, bit for bit.

    h_2 = 0 alone makes the 16 column-tile bounds bit-equal too (the column-tile order is the
    natural one), but the row-tile bounds still depend on x_0 through h_0, so the four row
    blocks of a tile are visited by their bounds and a tile's sums R1 / Q / N0 may be added in
    another order: that case is compared at 1e-11 max|c|^2."""
    varn, b = _batch(sbce, 4, 20)
    scale = np.abs(b["cons"]).max() ** 2
    assert _same_bits(sbce, b, _zeroed(b, 4, (0, 2)), varn)
    th = _zeroed(b, 4, (2,))
    for sph in ("1", "0"):
        m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
        m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="0", SBCE_ESTEP_SPHERE=sph)
        dm, dS = np.abs(m1 - m0).max(), np.abs(S1 - S0).max()
        print(f"h_2 = 0, sphere {sph}: bitwise {np.array_equal(m1, m0) and np.array_equal(S1, S0)}, "
              f"|dm| {dm:.2e} |dS| {dS:.2e}")
        assert dm < BAR * scale and dS < BAR * scale, (sph, dm, dS)


def test_deterministic(sbce):
    """Two E-steps at the same theta are bitwise equal (the moment-repeat freeze depends on it)."""
    for snr in (20, 0):
        varn, b = _batch(sbce, 4, snr)
        for th in (b["theta0"], _near_true(b)):
            for sph in ("1", "0"):
                m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
                m2, S2 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
                assert np.array_equal(m1, m2) and np.array_equal(S1, S2), (snr, sph)


def test_counters_follow_the_restatement(sbce):
    """cfg1 geometry (4 x 4, N_RIS 64, T_d 64, 4 trials, 20 dB) at theta_0, sweep only, tables
    always built: best-first runs fewer FP64 groups than the natural order, and both the groups at
    the screen and the FP64 groups are within 10 % of the CPU restatement in the device's order
    (the allowance of test_gpu_estep_tribound.py for rounding at the margins)."""
    varn = float(sbce.signal_model.snr_to_varn(20))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 64, 16, 64, 16, varn, seed=2)
    lib = sbce._lib.load_ab()
    cnt = {}
    for order in ("0", "1"):
        with sbce._lib.debug_env(SBCE_ESTEP_ORDER=order, SBCE_ESTEP_TRI="2", SBCE_ESTEP_SPHERE="0",
                                 SBCE_ESTEP_COUNT="1"):
            lib.sbce_debug_estep_groups(None, 1)
            lib.sbce_debug_estep_mfma(None, 1)
            sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], b["theta0"], varn, 4, "soft")
            g, m = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
            assert lib.sbce_debug_estep_groups(ctypes.byref(g), 0) == 0
            lib.sbce_debug_estep_mfma(ctypes.byref(m), 0)
            cnt[order] = (g.value, m.value // 8)       # FP64 group: STEPS * TU = 8 MFMAs
    ref = gb.count_groups(b, b["theta0"], varn, tri=True, order="device")
    nat = gb.count_groups(b, b["theta0"], varn, tri=True, order="natural")
    print(f"groups to the screen: ORDER=0 {cnt['0'][0]} (restatement {nat['screen']}), ORDER=1 {cnt['1'][0]} "
          f"(restatement {ref['screen']}); FP64 groups: ORDER=0 {cnt['0'][1]} ({nat['fp64']}), "
          f"ORDER=1 {cnt['1'][1]} ({ref['fp64']}) ({4 * 64} symbols)")
    assert cnt["1"][1] < cnt["0"][1]
    assert abs(cnt["1"][0] - ref["screen"]) <= 0.10 * ref["screen"]
    assert abs(cnt["1"][1] - ref["fp64"]) <= 0.10 * ref["fp64"]
