"""csrc/estep_pm.hip route by route against the extended-precision restatement tests/pm_ref.py.

rows (pm_ref.GRID; every case B = 3, theta_narrow and theta_wide, every arm of its row):
  1  estep_det_thread_kernel<1, NR, 4/5>        n_rx 1..8                 default, wave
  2  estep_det_thread_kernel<2, NR, 4/5>        n_rx 2..8 (MMSE also 1)   default, wave
  3  estep_pm_quad / estep_pm_thread<2/3, NR>   n_rx 2..8, |A| = 1        default (quad), t, q, wave
  4  estep_pm_kernel<2/3>, empty B, n_tx = 1                              default
  5  estep_pm_kernel<2/3>, lists of 2..64, n_tx 3..8, P = 1               default
  6  estep_pm_kernel<4/5>, n_tx 3..8, MMSE with n_rx < n_tx, P = 1        default
  7  estep_pm_kernel<6>                                                   default
The inputs' conditions (pm_ref.check_conditions: every decision margin >= 1e-6, cond <= 1e6, no
symbol left out) are asserted on the host before a case's first device call, so a device that
decides otherwise than the restatement is wrong, not unlucky.  Given equal decisions the bars are
derived (u = 2^-53):
  ZF / MMSE   m bitwise a table entry; |S - ref| <= 3 u max|c|^2
  PM          |m - ref| <= (JA + 1) u sum_j |x_j|;  |S - ref| <= (JA + 3) u sum_j |x_a||x_b|
  PM-soft     kappa = (P + n_tx + 4) u A_t / varn^2, A_t = max_j sum_r (|y_r| + sum_a |H_ra||x_a|)^2;
              |dm| <= (2 kappa + (JA + 6) u) max|c|, |dS| <= (same) max|c|^2; and the suite's
              1e-11 max|c|^2 beside it at <= 20 dB
  Gauss       pm_ref.GAUSS_C cond(A) u relative to max|m|, max|C| (the one measured constant)
The largest err / bound per row is printed (DESIGN section 6 records the MI355X run)."""
import numpy as np
import pytest

import pm_ref as pr

pytestmark = pytest.mark.gpu

U = pr.U
SOFT_TOL = 1e-11            # x max|c|^2, the suite's bar on posterior-weighted moments
DETECTOR = 4                # SBCE_STATUS_DETECTOR
_worst = {}                 # (row, what) -> largest err / bound


def _note(case, what, ratio):
    key = (case["row"], what)
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))


def _run(sbce, case, kind, mode, arm, varn=None, y_d=None, rows=slice(None), tile=1, status=False):
    """One device E-step of the case.  arm '' is the product library, any other the A/B build
    with SBCE_PM_IMPL set.  rows / tile: a sub-batch, repeated."""
    b = pr.batch(case)
    th, psi = pr.gauss_inputs(case, kind) if mode == "gauss" else (b["theta_" + kind], b["psi_d"])
    y = b["y_d"] if y_d is None else y_d
    rep = lambda a: np.tile(np.asarray(a)[rows], (tile,) + (1,) * (np.ndim(a) - 1))
    v = b["varn"] if varn is None else (rep(varn) if np.ndim(varn) else varn)

    def call():
        return sbce.estep_batch(rep(y), rep(psi), b["cons"], rep(th), v, case["n_tx"], mode,
                                case["r"], varx=case["varx"], return_status=status)
    if arm == "":
        return call()
    with sbce._lib.debug_env(SBCE_PM_IMPL=arm):
        return call()


def _ratio(err, bound):
    """max err / bound; a zero bound demands a zero error."""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=float), np.asarray(bound, dtype=float))
    out = np.zeros(err.shape)
    np.divide(err, bound, out=out, where=bound > 0)
    out[(bound == 0) & (err > 0)] = np.inf
    return float(out.max()) if out.size else 0.0


def _hold_det(case, ref, m, S, tag, sel=slice(None)):
    c2 = np.abs(pr.batch(case)["cons"]).max() ** 2
    assert np.array_equal(m[:, sel], ref["m"][:, sel]), (tag, "decisions")
    r = _ratio(np.abs(S - ref["S"])[:, sel], 3 * U * c2)
    _note(case, "det S", r)
    assert r <= 1, (tag, "S", r)


def _hold_list(case, ref, m, S, soft, varn, tag):
    b = pr.batch(case)
    cmax = np.abs(b["cons"]).max()
    JA = ref["lst"].shape[2]
    if not soft:
        rm = _ratio(np.abs(m - ref["m_u"]), (JA + 1) * U * ref["ax"])
        rs = _ratio(np.abs(S - ref["S_u"]), (JA + 3) * U * ref["axx"])
        _note(case, "pm m", rm)
        _note(case, "pm S", rs)
        assert rm <= 1 and rs <= 1, (tag, rm, rs)
        return
    s2 = (np.broadcast_to(varn, (pr.B,)) ** 2)[:, None]
    kappa = (b["P"] + case["n_tx"] + 4) * U * ref["kap_num"] / s2            # (B, T)
    dw = 2 * kappa + (JA + 6) * U
    em = np.abs(m - ref["m_s"]).max(axis=2)
    es = np.abs(S - ref["S_s"]).max(axis=(2, 3))
    rm, rs = _ratio(em, dw * cmax), _ratio(es, dw * cmax ** 2)
    _note(case, "pm_soft m", rm)
    _note(case, "pm_soft S", rs)
    print(f"{tag}: pm_soft err/bound m {rm:.3f} S {rs:.3f}; max err / max|c|^2 "
          f"{max(em.max(), es.max()) / cmax ** 2:.2e}")
    assert rm <= 1 and rs <= 1, (tag, rm, rs)
    if case["snr"] <= 20:
        assert em.max() <= SOFT_TOL * cmax ** 2 and es.max() <= SOFT_TOL * cmax ** 2, tag


def _hold_gauss(case, ref, m, S, tag):
    cond = ref["cond"].max(axis=1)
    for got, want, what in ((m, ref["m"], "gauss m"), (S, ref["C"], "gauss C")):
        flat = lambda a: np.abs(a).reshape(pr.B, -1).max(axis=1)
        r = _ratio(flat(got - want), pr.GAUSS_C * cond * U * flat(want))
        _note(case, what, r)
        assert r <= 1, (tag, what, r)


def _hold(case, kind, mode, m, S, tag, varn=None):
    ref = pr.reference(case, kind, mode, None if varn is None else varn)
    v = pr.batch(case)["varn"] if varn is None else np.asarray(varn)
    if mode in ("zf", "mmse"):
        _hold_det(case, ref, m, S, tag)
    elif mode == "gauss":
        _hold_gauss(case, ref, m, S, tag)
    else:
        _hold_list(case, ref, m, S, mode == "pm_soft", v, tag)
    return ref


def test_grid_reaches_every_instantiation():
    """Every (kernel, NR) instantiation launch_estep_pm can reach with n_rx >= n_tx (MMSE and
    Gauss below that too) is launched by a case of the grid (host restatement of the dispatch)."""
    missing = pr.reachable() - pr.covered()
    assert not missing, sorted(missing)


@pytest.mark.parametrize("case", pr.GRID, ids=lambda c: c["id"])
def test_route_vs_restatement(sbce, case):
    """Every arm and mode of the case, theta_narrow and theta_wide, against the restatement; the
    detector flag is set for exactly the trials that hold a symbol past the table (BPSK, n_tx >=
    2), whose moments are the documented `flat mod M^n_tx` row."""
    pr.check_conditions(case)
    for kind in ("narrow", "wide"):
        for mode in case["modes"]:
            for arm in case["arms"]:
                tag = (case["id"], kind, mode, arm)
                m, S, st = _run(sbce, case, kind, mode, arm, status=True)
                assert np.isfinite(m).all() and np.isfinite(S).all(), tag
                ref = _hold(case, kind, mode, m, S, tag)
                if mode in ("zf", "mmse"):
                    assert np.array_equal((st & DETECTOR) != 0, ref["over"].any(axis=1)), tag
                    if case["tab"] == "bpsk":
                        assert ref["over"].any(), tag
                else:
                    assert not (st & DETECTOR).any(), tag


@pytest.mark.parametrize("case", pr.TIE_CASES, ids=lambda c: c["id"])
def test_planted_exact_ties(sbce, case):
    """y_d = 0 on every second symbol: z is exactly 0, the four innermost points of the integer
    grids tie exactly and so do the streams; nearest_point's per-axis shortcut must hand over to
    the scan in table order: the decision is bitwise the restatement's first minimum at stream 0,
    in the thread and the wave kernel."""
    y, mask = pr.tie_inputs(case)
    pr.check_conditions(case, y_d=y, exempt=mask)
    for kind in ("narrow", "wide"):
        for mode in case["modes"]:
            ref = pr.reference(case, kind, mode, y_d=y)
            for arm in case["arms"]:
                tag = (case["id"], kind, mode, arm)
                m, S, st = _run(sbce, case, kind, mode, arm, y_d=y, status=True)
                assert np.array_equal(m[:, mask], ref["m"][:, mask]), (tag, "tie decisions")
                assert np.array_equal(S[:, mask], ref["S"][:, mask]), (tag, "tie S")
                _hold_det(case, ref, m, S, tag, sel=~mask)
                assert np.array_equal((st & DETECTOR) != 0, ref["over"].any(axis=1)), tag


@pytest.mark.parametrize("case", pr.VARN_CASES, ids=lambda c: c["id"])
def test_per_trial_noise(sbce, case):
    """A (B,) varn of (0.5, 1, 2) x nominal: MMSE and PM-soft hold each trial to the restatement
    at its own sigma and are bitwise a scalar call at that sigma; ZF and PM do not change."""
    v = pr.varn_vector(case)
    pr.check_conditions(case, varn=v)
    for kind in ("narrow", "wide"):
        for mode in case["modes"]:
            for arm in case["arms"]:
                tag = (case["id"], kind, mode, arm, "varn_t")
                m, S = _run(sbce, case, kind, mode, arm, varn=v)
                if mode in ("mmse", "pm_soft"):
                    _hold(case, kind, mode, m, S, tag, varn=v)
                    for i in range(pr.B):
                        m1, S1 = _run(sbce, case, kind, mode, arm, varn=float(v[i]),
                                      rows=slice(i, i + 1))
                        assert np.array_equal(m[i], m1[0]) and np.array_equal(S[i], S1[0]), (tag, i)
                else:
                    m0, S0 = _run(sbce, case, kind, mode, arm)
                    assert np.array_equal(m, m0) and np.array_equal(S, S0), tag


@pytest.mark.parametrize("case", pr.INDEP_CASES, ids=lambda c: c["id"])
def test_trials_are_independent(sbce, case):
    """The batch tiled to B = 300: every trial is bitwise its B = 1 result."""
    for mode in case["modes"]:
        m, S = _run(sbce, case, "wide", mode, "", tile=100)
        assert m.shape[0] == 300
        for i in range(pr.B):
            m1, S1 = _run(sbce, case, "wide", mode, "", rows=slice(i, i + 1))
            assert np.array_equal(m[i::pr.B], np.repeat(m1, 100, axis=0)), (case["id"], mode, i)
            assert np.array_equal(S[i::pr.B], np.repeat(S1, 100, axis=0)), (case["id"], mode, i)


def test_zz_report_largest_ratios():
    """Prints the largest err / bound per row (runs last in this file)."""
    for (row, what), r in sorted(_worst.items()):
        print(f"row {row} {what}: largest err / bound = {r:.3g}")
