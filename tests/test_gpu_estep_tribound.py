"""The V16 sweep's per-group bounds T_3 / T_1 (csrc/estep_sweep.hip build_tri, SBCE_ESTEP_TRI in the
A/B build: 0 off, 1 built once 4 groups of a symbol reached the screen -- the default -- and 2
built for every swept symbol).

A group the bounds skip holds no hypothesis within the running skip bound, so soft moments and
hard decisions must be BITWISE those of SBCE_ESTEP_TRI=0: with and without the sphere pass, in
front of the FP32 screen and of the bare FP64 test (SBCE_ESTEP_F32=0), at n_rx 2 and 3 (no
sphere pass; at n_rx = 2 the row bound's P_13 is 0 while P_1 and P_3 are not), on degenerate
columns and on scaled data.  The counters (SBCE_ESTEP_COUNT=1) show that the bounds do remove
groups and agree with the CPU restatement tools/e0_group_bounds.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import e0_group_bounds as gb  # noqa: E402

pytestmark = pytest.mark.gpu


def _near_true(b):
    return b["h"] + 0.05 * b["theta0"] / np.abs(b["theta0"]).max()


def _both(sbce, b, th, varn, y=None):
    y = b["y_d"] if y is None else y
    return [sbce.estep_batch(y, b["psi_d"], b["cons"], th, varn, 4, m) for m in ("soft", "hard")]


def _assert_same(res, ref, key):
    for (x1, y1), (x0, y0) in zip(res, ref):
        assert np.array_equal(x1, x0) and np.array_equal(y1, y0), key


@pytest.mark.parametrize("snr", [30, 20, 10, 0, -5])
@pytest.mark.parametrize("n_rx", [2, 3, 4, 8])
def test_group_bounds_are_bitwise_neutral(sbce, n_rx, snr):
    varn = float(sbce.signal_model.snr_to_varn(snr))
    b = sbce.signal_model.synthetic_batch(4, 4, n_rx, 8, 16, 32, 16, varn, seed=70 + snr + n_rx)
    for th in (b["theta0"], _near_true(b)):
        for sph in ("1", "0"):
            for f32 in ("1", "0"):
                res = {}
                for tri in ("0", "1", "2"):
                    with sbce._lib.debug_env(SBCE_ESTEP_TRI=tri, SBCE_ESTEP_SPHERE=sph,
                                             SBCE_ESTEP_F32=f32):
                        res[tri] = _both(sbce, b, th, varn)
                _assert_same(res["1"], res["0"], (n_rx, snr, sph, f32, 1))
                _assert_same(res["2"], res["0"], (n_rx, snr, sph, f32, 2))


def _streams(b, n_rx):
    """theta as (B, P, n_tx, n_rx): H_eff's column q is theta[:, :, q, :] weighted by psi."""
    return b["theta0"].reshape(b["theta0"].shape[0], -1, 4, n_rx).copy()


@pytest.mark.parametrize("case", ["zero1", "zero3", "zero13", "same13"])
@pytest.mark.parametrize("n_rx", [3, 4])
def test_degenerate_columns(sbce, n_rx, case):
    """A zero column h_q leaves that bound at 0 (nothing skipped); h_1 = h_3 leaves each bound a
    valid one (P_3 h_1 = 0).  Bitwise TRI=0 and finite, where TRI=0 is finite."""
    varn = float(sbce.signal_model.snr_to_varn(20))
    b = sbce.signal_model.synthetic_batch(4, 4, n_rx, 8, 16, 32, 16, varn, seed=90 + n_rx)
    th = _streams(b, n_rx)
    if case in ("zero1", "zero13"):
        th[:, :, 1, :] = 0.0
    if case in ("zero3", "zero13"):
        th[:, :, 3, :] = 0.0
    if case == "same13":
        th[:, :, 3, :] = th[:, :, 1, :]
    th = th.reshape(b["theta0"].shape)
    for sph in ("1", "0"):
        res = {}
        for tri in ("0", "1", "2"):
            with sbce._lib.debug_env(SBCE_ESTEP_TRI=tri, SBCE_ESTEP_SPHERE=sph):
                res[tri] = _both(sbce, b, th, varn)
        for tri in ("1", "2"):
            _assert_same(res[tri], res["0"], (case, sph, tri))
            for m, S in res[tri]:
                assert np.isfinite(m).all() and np.isfinite(S).all(), (case, sph, tri)


@pytest.mark.parametrize("case", ["all_varn1e12", "all_varn1e6", "theta0"])
def test_scaled_data(sbce, case):
    """The margins scale with the data: y and theta times 1e6 with varn times 1e12, the same with
    varn times 1e6 (the device squares varn: then every distance and the threshold scale alike),
    and theta times 1e6 alone (a far-off candidate).  Bitwise TRI=0."""
    varn = float(sbce.signal_model.snr_to_varn(20))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 8, 16, 32, 16, varn, seed=95)
    for th0 in (b["theta0"], _near_true(b)):
        y, th, v = {"all_varn1e12": (b["y_d"] * 1e6, th0 * 1e6, varn * 1e12),
                    "all_varn1e6": (b["y_d"] * 1e6, th0 * 1e6, varn * 1e6),
                    "theta0": (b["y_d"], th0 * 1e6, varn)}[case]
        for sph in ("1", "0"):
            res = {}
            for tri in ("0", "1", "2"):
                with sbce._lib.debug_env(SBCE_ESTEP_TRI=tri, SBCE_ESTEP_SPHERE=sph):
                    res[tri] = _both(sbce, b, th, v, y=y)
            _assert_same(res["1"], res["0"], (case, sph, 1))
            _assert_same(res["2"], res["0"], (case, sph, 2))


def test_counters_cfg1_geometry(sbce):
    """cfg1 geometry (4 x 4, N_RIS 64, T_d 64, 4 trials, 20 dB) at theta_0, sweep only: the bounds
    remove groups from the screen, add no FP64 group, and the device's count of groups reaching
    the screen is within 10 % of the CPU restatement's with the device's margins (the allowance
    covers rounding at the margin: both count the same thing).
    MI355X: recorded in profiles/tribound/README.md."""
    varn = float(sbce.signal_model.snr_to_varn(20))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 64, 16, 64, 16, varn, seed=2)
    lib = sbce._lib.load_ab()
    cnt = {}
    for tri in ("0", "2"):
        with sbce._lib.debug_env(SBCE_ESTEP_TRI=tri, SBCE_ESTEP_SPHERE="0", SBCE_ESTEP_COUNT="1"):
            lib.sbce_debug_estep_groups(None, 1)
            lib.sbce_debug_estep_mfma(None, 1)
            sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], b["theta0"], varn, 4, "soft")
            g, m = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
            assert lib.sbce_debug_estep_groups(ctypes.byref(g), 0) == 0
            lib.sbce_debug_estep_mfma(ctypes.byref(m), 0)
            cnt[tri] = (g.value, m.value // 8)       # FP64 group: STEPS * TU = 8 MFMAs
    ref = gb.count_groups(b, b["theta0"], varn, tri=True)
    print(f"groups to the screen: TRI=0 {cnt['0'][0]}, TRI=2 {cnt['2'][0]}, restatement "
          f"{ref['screen']}; FP64 groups: TRI=0 {cnt['0'][1]}, TRI=2 {cnt['2'][1]}, "
          f"restatement {ref['fp64']} ({4 * 64} symbols)")
    assert cnt["2"][0] < cnt["0"][0]
    assert cnt["2"][1] <= cnt["0"][1]
    assert abs(cnt["2"][0] - ref["screen"]) <= 0.10 * ref["screen"]
