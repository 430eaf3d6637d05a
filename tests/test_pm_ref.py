"""CPU tier of the list / detector / Gauss E-step tests: the extended-precision restatement
tests/pm_ref.py against the float64 oracles on the whole grid of tests/test_gpu_estep_list.py, its
margin functions on constructed ties and a hand-made case, and the grid's own conditions and
coverage.  No GPU."""
import numpy as np
import pytest

import estep_ref as er
import pm_ref as pr

IDS = [c["id"] for c in pr.GRID]


def _scale(case):
    return np.abs(pr.table(case["tab"])).max() ** 2


@pytest.mark.parametrize("case", pr.by_row(3) + pr.by_row(4) + pr.by_row(5),
                         ids=lambda c: c["id"])
def test_list_restatement_equals_oracle(case):
    """m, S (uniform and posterior weights) equal oracle.pm.pm_moments to 1e-12 max|c|^2, and the
    stream order equals _stream_order's, on every list case of the grid."""
    from oracle.pm import pm_moments, _stream_order
    b = pr.batch(case)
    n_tx, n_rx, tol = case["n_tx"], case["n_rx"], 1e-12 * _scale(case)
    for kind in ("narrow", "wide"):
        ref = pr.reference(case, kind, "pm")
        th = b["theta_" + kind]
        for i in range(pr.B):
            for soft, sfx in ((False, "_u"), (True, "_s")):
                m0, S0 = pm_moments(th[i], b["y_d"][i], b["psi_d"][i].T, b["cons"], n_tx, n_rx,
                                    case["r"], b["varn"], soft)
                assert np.abs(ref["m" + sfx][i] - m0).max() <= tol, (kind, i, soft)
                assert np.abs(ref["S" + sfx][i] - S0).max() <= tol, (kind, i, soft)
            Ho = pr.channels(th[i], b["psi_d"][i], n_tx, n_rx)[1].astype(np.complex128)
            for t in range(case["T_d"]):
                assert _stream_order(Ho[t]) == ref["order"][i, t].tolist(), (kind, i, t)


@pytest.mark.parametrize("case", pr.by_row(1) + pr.by_row(2) + pr.by_row(6),
                         ids=lambda c: c["id"])
def test_detector_restatement_equals_oracle(case):
    """The decided rows equal oracle.detectors.detector_moments' (nearest_symbol_ecul as written
    where n_tx <= 3, its closed form above), S to 1e-12 max|c|^2, and the oracle's IndexError
    symbols are exactly the restatement's flat >= M^n_tx symbols."""
    from oracle.detectors import detector_moments
    from oracle.em_reduced import aps_from_cons
    b = pr.batch(case)
    n_tx, n_rx, cons = case["n_tx"], case["n_rx"], b["cons"]
    aps = aps_from_cons(cons, n_tx) if n_tx <= 3 else None
    tol = 1e-12 * _scale(case)
    for kind in ("narrow", "wide"):
        th = b["theta_" + kind]
        for mode in case["modes"]:
            ref = pr.reference(case, kind, mode)
            for i in range(pr.B):
                for t in range(case["T_d"]):
                    try:
                        m0, S0 = detector_moments(th[i], b["y_d"][i, t:t + 1],
                                                  b["psi_d"][i, t:t + 1].T, aps, b["varn"], n_tx,
                                                  n_rx, mode, cons=cons)
                        raised = False
                    except IndexError:
                        raised = True
                    assert raised == bool(ref["over"][i, t]), (kind, mode, i, t)
                    if not raised:
                        assert np.array_equal(ref["m"][i, t], m0[0]), (kind, mode, i, t)
                        assert np.abs(ref["S"][i, t] - S0[0]).max() <= tol
    if case["tab"] == "bpsk":
        assert ref["over"].any() and not ref["over"].all()


@pytest.mark.parametrize("case", pr.by_row(7), ids=lambda c: c["id"])
def test_gauss_restatement_equals_oracle(case):
    from oracle.gaussian import gaussian_moments
    b = pr.batch(case)
    n_tx, n_rx = case["n_tx"], case["n_rx"]
    for kind in ("narrow", "wide"):
        ref = pr.reference(case, kind, "gauss")
        th, psi = pr.gauss_inputs(case, kind)
        for i in range(pr.B):
            Hr = th[i].reshape(case["N"] * n_tx, n_rx).T
            m0, C0 = gaussian_moments(Hr, b["y_d"][i], psi[i].T, b["varn"], case["varx"], n_tx)
            assert np.abs(ref["m"][i] - m0).max() <= 1e-12 * _scale(case)
            assert np.abs(ref["C"][i] - C0).max() <= 1e-12 * _scale(case)


def test_gauss_constant():
    """GAUSS_C is 4 x the largest error of numpy's float64 evaluation, in units of cond(A) 2^-53
    max|.|, rounded up; the measured ratio is printed."""
    worst = 0.0
    for case in pr.by_row(7):
        b = pr.batch(case)
        for kind in ("narrow", "wide"):
            ref = pr.reference(case, kind, "gauss")
            th, psi = pr.gauss_inputs(case, kind)
            for i in range(pr.B):
                m, C = pr.gauss_float64(th[i], b["y_d"][i], psi[i], b["varn"], case["varx"],
                                        case["n_tx"])
                for got, want in ((m, ref["m"][i]), (C, ref["C"][i])):
                    unit = ref["cond"][i].max() * pr.U * np.abs(want).max()
                    worst = max(worst, np.abs(got - want).max() / unit)
    print(f"float64 Gauss evaluation: largest err / (cond 2^-53 max) = {worst:.3f}")
    assert 4 * worst <= pr.GAUSS_C <= 8 * worst + 1


def test_herm_inv_is_an_inverse():
    g = np.random.default_rng(0)
    for n in (1, 2, 5, 8):
        H = g.normal(size=(4, n + 1, n)) + 1j * g.normal(size=(4, n + 1, n))
        G = pr._gram(H.astype(pr.CLD))
        E = np.einsum("tuv,tvw->tuw", pr.herm_inv(G), G) - np.eye(n)
        assert np.abs(E).max() < 1e-15


def test_margins_on_ties_and_a_hand_case():
    """gap_min / gap_max are 0 on exact ties (also 0 / 0) and inf without a rival; on H = diag(1,
    2) (P = 1), y = (0.5, 0.4), BPSK, every margin is the hand-computed one."""
    assert pr.gap_min(np.array([3.0, 2.0, 2.0])) == 0 and pr.gap_max(np.array([5.0, 1.0, 5.0])) == 0
    assert pr.gap_min(np.array([0.0, 0.0, 1.0])) == 0 and pr.gap_min(np.array([7.0])) == np.inf
    assert pr.gap_min(np.array([4.0, 1.0, 2.0])) == 0.5 and pr.gap_max(np.array([4.0, 1.0, 2.0])) == 0.5
    cons = er.table("bpsk")
    theta = np.array([1.0, 0.0, 0.0, 2.0], dtype=complex)          # [a * n_rx + r]
    y = np.array([[0.5, 0.4]], dtype=complex)
    psi = np.ones((1, 1), dtype=complex)
    d = pr.det_moments(theta, y, psi, cons, 1.0, 2, "zf")           # z = (0.5, 0.2)
    assert np.allclose(d["g_near"][0], [(2.25 - 0.25) / 2.25, (1.44 - 0.64) / 1.44], rtol=1e-15)
    assert np.isclose(d["g_stream"][0], (0.64 - 0.25) / 0.64, rtol=1e-15)
    assert d["flat"][0] == 0 and not d["over"][0] and np.array_equal(d["m"][0], [1, 1])
    p = pr.list_moments(theta, y, psi, cons, 1.0, 2, 0)             # diag(G^-1) = (1, 1/4)
    assert np.isclose(p["g_order"][0, 0], 0.75, rtol=1e-15) and p["order"][0].tolist() == [0, 1]
    # candidate a = +1 on stream 0: z_1 = 0.2 -> 0.64 against 1.44
    assert np.isclose(p["g_near"][0, 0, 0], (1.44 - 0.64) / 1.44, rtol=1e-15)
    # an exact greedy tie takes the FIRST maximum; an exact nearest-point tie the first minimum
    th2 = np.array([1.0, 0.0, 0.0, 1.0], dtype=complex)
    q = pr.list_moments(th2, np.zeros((1, 2), dtype=complex), psi, cons, 1.0, 2, 0)
    assert q["g_order"][0, 0] == 0 and q["order"][0].tolist() == [0, 1]
    assert np.all(q["g_near"] == 0) and np.all(q["lst"][0, :, 1] == 0)


@pytest.mark.parametrize("case", pr.TIE_CASES, ids=lambda c: c["id"])
def test_planted_ties_are_exact_ties(case):
    """On the zeroed symbols every nearest-point and stream margin is exactly 0, the decision is
    the first of the four innermost points in table order at stream 0; the other symbols meet the
    grid's conditions."""
    y, mask = pr.tie_inputs(case)
    pr.check_conditions(case, y_d=y, exempt=mask)
    cons = pr.batch(case)["cons"]
    s0 = int(np.argmin(np.abs(cons)))                      # first minimum = first inner point
    if case["tab"] == "qam64_perm":                        # not what a search in grid order finds
        assert cons[s0] != -1 - 1j
    n_tx = case["n_tx"]
    want = pr.flat_index(0, s0, n_tx)
    for mode in case["modes"]:
        ref = pr.reference(case, "wide", mode, y_d=y)
        assert np.all(ref["flat"][:, mask] == want) and not ref["over"][:, mask].any()


@pytest.mark.parametrize("case", pr.GRID, ids=IDS)
def test_grid_conditions(case):
    pr.check_conditions(case)


@pytest.mark.parametrize("case", pr.VARN_CASES, ids=lambda c: c["id"])
def test_grid_conditions_per_trial_noise(case):
    pr.check_conditions(case, varn=pr.varn_vector(case))


def test_grid_seeds_shapes_and_coverage():
    """Seeds are grid positions (or the recorded re-draws), every case has B = 3 and the T_d of
    its row, each table of the n_tx = 2 cycle meets two n_rx, and every instantiation that
    launch_estep_pm can reach is launched by some case."""
    for i, c in enumerate(pr.GRID):
        assert c["pos"] == i and c["seed"] == pr.RESEED.get(i, i)
        assert c["T_d"] == (23 if c["n_tx"] <= 2 else 6) or c["row"] == 7
    for row in (2, 3):
        for tab in pr._CYCLE:
            assert len({c["n_rx"] for c in pr.by_row(row) if c["tab"] == tab}) >= 2, (row, tab)
    missing = pr.reachable() - pr.covered()
    assert not missing, sorted(missing)
    assert pr.route("pm", 2, 4, 64, 1, "", 96 * 1024) == "pm_thread<2,4>"
    assert pr.route("pm", 2, 4, 4, 2, "", 69) == "pm_wave<2>"
    assert pr.route("zf", 3, 4, 4, 0, "", 69) == "pm_wave<4>"
