"""The two-pass V16 soft sweep (csrc/estep_sweep.hip): the search keeps only the running minimum
and a 64-bit mask of the tile groups that passed its FP64 test; a second pass recomputes the marked
groups in natural order and sums the weights exp((d_min - d) / s^2) against the final minimum.
SBCE_ESTEP_TWOPASS=0 in the A/B build is the one-pass sweep (online shift, rescaled sums).

Both arms sum the same posterior: the moments agree to the project's bar for two writers of one
posterior, 1e-11 max|c|^2, and to the oracle's enumeration of all 65,536 hypotheses.  The second
pass does not depend on the search order (bitwise equal under SBCE_ESTEP_ORDER=0 / 1), the search
is the one-pass sweep's (equal counters), the hard decision never runs the two-pass body (bitwise
equal between the arms) and the E-step stays deterministic, so the moment-repeat rule of sbce_em
still finds repeats."""
import ctypes

import numpy as np
import pytest

from oracle.em_reduced import estep_moments

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


def _same_bits(a, b):
    """Symbols (of 128) whose m and S are bitwise equal in both arms."""
    m1, S1 = a
    m0, S0 = b
    eq = (m1 == m0).all(axis=-1) & (S1 == S0).all(axis=(-1, -2))
    return int(eq.sum())


@pytest.mark.parametrize("snr", [30, 20, 10, 0, -5])
@pytest.mark.parametrize("n_rx", [3, 4, 8])
def test_same_posterior(sbce, n_rx, snr):
    varn, b = _batch(sbce, n_rx, snr)
    scale = np.abs(b["cons"]).max() ** 2
    for name, th in (("theta0", b["theta0"]), ("near", _near_true(b))):
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="0", SBCE_ESTEP_SPHERE=sph)
            dm, dS = np.abs(m1 - m0).max(), np.abs(S1 - S0).max()
            print(f"n_rx {n_rx} snr {snr} {name} sphere {sph}: |dm| {dm:.2e} |dS| {dS:.2e} "
                  f"(bar {BAR * scale:.2e}), bitwise-equal symbols {_same_bits((m1, S1), (m0, S0))} of 128")
            assert np.isfinite(m1).all() and np.isfinite(S1).all()
            assert dm < BAR * scale and dS < BAR * scale, (n_rx, snr, name, sph, dm, dS)


@pytest.mark.parametrize("snr", [20, 0])
def test_against_the_oracle_enumeration(sbce, snr):
    """theta_0, n_rx = 4, at 20 dB and at 0 dB (every group is marked): the two-pass sweep against
    all 65,536 hypotheses per symbol."""
    varn, b = _batch(sbce, 4, snr)
    scale = np.abs(b["cons"]).max() ** 2
    aps = sbce.qam.all_possible_symbols(b["cons"], 4)
    ref = [estep_moments(b["theta0"][i], b["y_d"][i], b["psi_d"][i].T, aps, varn)[:2] for i in range(4)]
    for sph in ("1", "0"):
        m, S = _estep(sbce, b, b["theta0"], varn, "soft", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
        for i, (m0, S0) in enumerate(ref):
            dm, dS = np.abs(m[i] - m0).max(), np.abs(S[i] - S0).max()
            print(f"snr {snr} sphere {sph} trial {i}: |dm| {dm:.2e} |dS| {dS:.2e} (bar {BAR * scale:.2e})")
            assert dm < BAR * scale and dS < BAR * scale, (snr, sph, i, dm, dS)


@pytest.mark.parametrize("snr", [20, 10, 0])
@pytest.mark.parametrize("n_rx", [3, 4, 8])
def test_search_order_leaves_no_trace(sbce, n_rx, snr):
    """The second pass runs in natural order whatever order the search took: bitwise equal."""
    varn, b = _batch(sbce, n_rx, snr)
    for th in (b["theta0"], _near_true(b)):
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_ORDER="0", SBCE_ESTEP_SPHERE=sph)
            assert np.array_equal(m1, m0) and np.array_equal(S1, S0), (n_rx, snr, sph)


def _zeroed(b, n_rx, streams):
    th = b["theta0"].reshape(b["theta0"].shape[0], -1, 4, n_rx).copy()
    for q in streams:
        th[:, :, q, :] = 0.0
    return th.reshape(b["theta0"].shape)


def test_ties(sbce):
    """h_0 = h_2 = 0 (every bound ties) and n_rx = 2 (every bound is 0): finite, and within the bar
    of the one-pass arm."""
    cases = []
    varn, b = _batch(sbce, 4, 20)
    cases.append(("h0=h2=0", varn, b, _zeroed(b, 4, (0, 2))))
    for snr in (20, 0):
        varn, b = _batch(sbce, 2, snr)
        cases.append((f"n_rx 2, {snr} dB", varn, b, b["theta0"]))
        cases.append((f"n_rx 2, {snr} dB, near", varn, b, _near_true(b)))
    for name, varn, b, th in cases:
        scale = np.abs(b["cons"]).max() ** 2
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="0", SBCE_ESTEP_SPHERE=sph)
            dm, dS = np.abs(m1 - m0).max(), np.abs(S1 - S0).max()
            print(f"{name}, sphere {sph}: |dm| {dm:.2e} |dS| {dS:.2e} (bar {BAR * scale:.2e})")
            assert np.isfinite(m1).all() and np.isfinite(S1).all()
            assert dm < BAR * scale and dS < BAR * scale, (name, sph, dm, dS)


def test_deterministic(sbce):
    """Two E-steps at the same theta are bitwise equal (the moment-repeat freeze depends on it)."""
    for snr in (20, 0):
        varn, b = _batch(sbce, 4, snr)
        for th in (b["theta0"], _near_true(b)):
            for sph in ("1", "0"):
                m1, S1 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
                m2, S2 = _estep(sbce, b, th, varn, "soft", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
                assert np.array_equal(m1, m2) and np.array_equal(S1, S2), (snr, sph)


def test_a_repeated_estep_flags_no_change(sbce):
    """30 dB, 12 EM iterations, sphere pass off so that the sweep writes every symbol: the armed
    E-step of a trial at its fixed point repeats its moments bit for bit, flags no change, and
    sbce_em skips that trial's M-step (counted by the A/B build)."""
    varn = float(sbce.signal_model.snr_to_varn(30))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 8, 16, 32, 16, varn, seed=104)
    with sbce._lib.debug_env(SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE="0") as lib:
        assert lib.sbce_debug_momskip(None, 1) == 0
        r = sbce.em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], varn, 12, b["theta0"],
                          mode="soft")
        n = ctypes.c_ulonglong(0)
        assert lib.sbce_debug_momskip(ctypes.byref(n), 0) == 0
    print(f"M-steps skipped on repeated moments: {n.value}")
    assert np.isfinite(r["theta"].view(float)).all()
    assert n.value >= 1


def _counters(sbce, b, varn, twopass):
    lib = sbce._lib.load_ab()
    with sbce._lib.debug_env(SBCE_ESTEP_TWOPASS=twopass, SBCE_ESTEP_SPHERE="0", SBCE_ESTEP_COUNT="1"):
        lib.sbce_debug_estep_groups(None, 1)
        lib.sbce_debug_estep_mfma(None, 1)
        lib.sbce_debug_estep_pass2(None, 1)
        sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], b["theta0"], varn, 4, "soft")
        g, m, p = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        assert lib.sbce_debug_estep_groups(ctypes.byref(g), 0) == 0
        assert lib.sbce_debug_estep_mfma(ctypes.byref(m), 0) == 0
        assert lib.sbce_debug_estep_pass2(ctypes.byref(p), 0) == 0
    return g.value, m.value, p.value


@pytest.mark.parametrize("snr", [20, 0])
def test_counters(sbce, snr):
    """The search is the one-pass sweep's: the groups at the screen and the FP64 MFMAs are equal
    between the arms.  The second pass recomputes at most the search's FP64 groups, at least one
    per symbol, and the one-pass arm none."""
    varn, b = _batch(sbce, 4, snr)
    g1, m1, p1 = _counters(sbce, b, varn, "1")
    g0, m0, p0 = _counters(sbce, b, varn, "0")
    print(f"snr {snr}: to the screen {g1} / {g0}, FP64 MFMAs {m1} / {m0}, second-pass groups {p1} / {p0}")
    assert g1 == g0 and m1 == m0
    assert p0 == 0 and 128 <= p1 <= m1 // 8


@pytest.mark.parametrize("snr", [20, 0])
@pytest.mark.parametrize("n_rx", [3, 4, 8])
def test_hard_mode_is_untouched(sbce, n_rx, snr):
    varn, b = _batch(sbce, n_rx, snr)
    for th in (b["theta0"], _near_true(b)):
        for sph in ("1", "0"):
            m1, S1 = _estep(sbce, b, th, varn, "hard", SBCE_ESTEP_TWOPASS="1", SBCE_ESTEP_SPHERE=sph)
            m0, S0 = _estep(sbce, b, th, varn, "hard", SBCE_ESTEP_TWOPASS="0", SBCE_ESTEP_SPHERE=sph)
            assert np.array_equal(m1, m0) and np.array_equal(S1, S0), (n_rx, snr, sph)
