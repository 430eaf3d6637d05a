"""GPU tier: the M-step's R and B^H builds, route by route, against the extended-precision
restatement tests/mstep_ref.py -- every kernel launch_mstep_build, launch_rbuild_herm and
launch_mstep_small can select, n_tx 1..8, with general moments (distinct diagonals, fully complex
off-diagonals) and an ELEMENTWISE bound derived from the operation count, not measured:

    |dev - ref| <= (T_p + T_d + 8) 2^-53 abs_sum        (mstep_ref.bound)

beside the rel() < 1e-13 the earlier build tests hold.  Every test prints its largest
err / bound; run with -s to read them (DESIGN.md section 6 records the figures).

Routes (host restatements below, asserted against the grid itself):
  R:   rbuild_herm<4,4,16,68> (n_tx 4, P <= 68), <4,4,32,0> (69..130), <4,4,8,0> (P >= 131),
       rbuild_herm<8,1,16,68> (n_tx 8), rbuild_kernel<1,2,3> and rbuild_wide_kernel<5,6,7>
       (L > 64), rbuild_kernel<4> / rbuild_wide_kernel<8> gated on a non-Kronecker trial, and the
       one-workgroup build (L <= 64, n_tx not 4 or 8) in its four arms.
  B^H: rhs_dma_kernel (L <= 512, two chunk buffers fit 64 KB: 16-symbol chunks at P <= 128,
       4-symbol chunks above), rhs_lds_kernel (they do not fit), rhs_kernel (L > 512).
"""
import functools

import numpy as np
import pytest

import mstep_ref as mr
from conftest import rel

pytestmark = pytest.mark.gpu

TP, TD = 3, 19                  # the pilot / data boundary inside the first chunk of every route
SEED = 20


# ------------------------------------------------------------------ host restatements of the dispatch
def r_route(n_tx, P):
    L = P * n_tx
    if n_tx == 4:
        return "herm<4,4,16,68>" if P <= 68 else "herm<4,4,32,0>" if P <= 130 else "herm<4,4,8,0>"
    if n_tx == 8:
        return "herm<8,1,16,68>"
    if L <= 64:
        return "small"
    return f"rbuild<{n_tx}>" if n_tx <= 3 else f"wide<{n_tx}>"


def rhs_route(n_tx, n_rx, P):
    """launch_mstep_build's B^H kernel (the batched path): (kernel, symbols per chunk)."""
    if P * n_tx > 512:
        return "rhs_kernel", 0
    tcr = 16 if P <= 128 else 4
    fits = 2 * tcr * (P + n_tx + n_rx) * 16 <= 64 * 1024
    return ("rhs_dma" if fits else "rhs_lds"), tcr


# ------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def problem(B, n_tx, n_rx, P, T_p, T_d, broken=None):
    """The batch and its extended-precision reference, computed once and shared: read only."""
    b = mr.general_batch(B, n_tx, n_rx, P, T_p, T_d, SEED, break_trial=broken)
    return b, mr.batch_ref(b)


def run(sbce, b, env=None, **kw):
    args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], b["m"], b["S"], 1.0)
    if env is None:
        return sbce.mstep_batch(*args, **kw)
    with sbce._lib.debug_env(**env):
        return sbce.mstep_batch(*args, **kw)


def check_build(b, ref, out, label):
    """Every trial's R and B^H under the elementwise bound and the relative one; theta finite
    (R may be singular at the edge symbol counts).  Returns the largest err / bound."""
    th, R, rhs, st = out
    T_p, T_d = b["T_p"], b["T_d"]
    worst = 0.0
    for i, (R0, rhs0, R_abs, rhs_abs) in enumerate(ref):
        rr = mr.ratio(R[i], R0, T_p, T_d, R_abs)
        rb = mr.ratio(rhs[i], rhs0, T_p, T_d, rhs_abs)
        worst = max(worst, rr, rb)
        print(f"[mstep-build] {label} trial {i}: err/bound R {rr:.3f} rhs {rb:.3f}")
        assert rr <= 1.0, (label, i, rr)
        assert rb <= 1.0, (label, i, rb)
        assert rel(R[i], R0.astype(np.complex128)) < 1e-13, (label, i)
        assert rel(rhs[i], rhs0.astype(np.complex128)) < 1e-13, (label, i)
    assert np.isfinite(th).all(), label
    return worst


def label_of(n_tx, n_rx, P, T_p=TP, T_d=TD):
    k, tcr = rhs_route(n_tx, n_rx, P)
    return (f"{r_route(n_tx, P)} + {k}{tcr or ''}<{n_rx}> ({n_tx},{n_rx},{P}) "
            f"T_p={T_p} T_d={T_d}")


# ------------------------------------------------------------------ the grid (rows 1-6)
ROWS = {
    # row: (R route, [(n_tx, n_rx, P, B)])
    1: ("herm<4,4,16,68>", [(4, 1, 1, 3), (4, 2, 22, 3), (4, 3, 23, 3), (4, 4, 33, 9),   # B = 9: the
                            (4, 2, 64, 3), (4, 4, 65, 3), (4, 1, 68, 3)]),   # b >= B guard, 2nd group of 8
    2: ("herm<4,4,32,0>", [(4, 4, 69, 3), (4, 3, 100, 3), (4, 8, 128, 3), (4, 2, 130, 3)]),
    3: ("herm<4,4,8,0>", [(4, 2, 131, 3), (4, 2, 258, 1), (4, 1, 300, 1)]),
    4: ("herm<8,1,16,68>", [(8, 1, 1, 3), (8, 2, 10, 3), (8, 3, 11, 3), (8, 4, 64, 3),
                            (8, 8, 65, 3), (8, 2, 66, 3), (8, 3, 81, 3)]),
    5: ("rbuild", [(1, 1, 65, 3), (1, 8, 300, 3), (2, 5, 40, 3), (2, 2, 256, 3), (3, 6, 22, 3),
                   (3, 7, 170, 3), (3, 2, 201, 3), (1, 3, 600, 3)]),
    6: ("wide", [(5, 4, 13, 3), (5, 3, 20, 3), (6, 5, 11, 3), (6, 5, 30, 3), (7, 2, 10, 3),
                 (7, 2, 73, 3), (5, 3, 103, 3), (6, 2, 86, 3)]),
}
GRID = [(row, *s) for row, (_, shapes) in ROWS.items() for s in shapes]
# B^H routes beside the rows': rhs_lds_kernel at its boundary, rhs_dma_kernel's 4-symbol chunks
RHS_EXTRA = [(2, 2, 124), (2, 2, 125), (1, 1, 128), (4, 8, 128),
             (1, 3, 129), (2, 4, 256), (3, 5, 170), (1, 2, 512)]


def test_grid_covers_the_routes_it_names():
    """The rows reach the kernels they are named for (the dispatch restated above), the
    Hermitian build's four staging layouts with the largest staged count, every n_rx on
    rhs_dma_kernel, both sides of rhs_lds_kernel's boundary and the 4-symbol chunks."""
    for row, (route, shapes) in ROWS.items():
        for n_tx, n_rx, P, B in shapes:
            assert r_route(n_tx, P).startswith(route), (row, n_tx, P)
    for row, ppb, count in ((3, 256, 257), (4, 64, 65)):
        segs = [mr.herm_segments(P, ppb) for _, _, P, _ in ROWS[row][1]]
        assert set().union(*(s["layouts"] for s in segs)) == set(mr.LAYOUTS), row
        assert max(s["count"] for s in segs) == count, row
    # P >= 65 at n_tx = 4: more than 64 staged phases, the second DMA segment of the STR = 68 image
    assert max(mr.herm_segments(P, 256)["count"] for _, _, P, _ in ROWS[1][1]) == 68
    assert {mr.herm_segments(P, 256)["count"] > 64 for _, _, P, _ in ROWS[1][1]} == {False, True}
    dma = {n_rx for _, n_tx, n_rx, P, _ in GRID if rhs_route(n_tx, n_rx, P)[0] == "rhs_dma"}
    assert dma == set(range(1, 9))
    assert {rhs_route(n_tx, n_rx, P)[0] for _, n_tx, n_rx, P, _ in GRID} == \
        {"rhs_dma", "rhs_lds", "rhs_kernel"}
    assert [rhs_route(*s) for s in RHS_EXTRA] == [
        ("rhs_dma", 16), ("rhs_lds", 16), ("rhs_lds", 16), ("rhs_lds", 16),
        ("rhs_dma", 4), ("rhs_dma", 4), ("rhs_dma", 4),
        ("rhs_lds", 4)]     # (1,2,512): P + n_tx + n_rx = 515 > 512, the single-buffer kernel


@pytest.mark.parametrize("row,n_tx,n_rx,P,B", GRID)
def test_build_grid(sbce, row, n_tx, n_rx, P, B):
    b, ref = problem(B, n_tx, n_rx, P, TP, TD)
    check_build(b, ref, run(sbce, b), f"row {row} " + label_of(n_tx, n_rx, P))


@pytest.mark.parametrize("n_tx,n_rx,P", RHS_EXTRA)
def test_rhs_routes(sbce, n_tx, n_rx, P):
    b, ref = problem(3, n_tx, n_rx, P, TP, TD)
    check_build(b, ref, run(sbce, b), "rhs " + label_of(n_tx, n_rx, P))


# ------------------------------------------------------------------ symbol-count edges
def _t_edges(tc):
    """(T_p, T_d) with T = T_p + T_d in {1 + 1, TC - 1, TC, TC + 1, 2 TC + 3}, T_p in {1, 3}."""
    return [(1, 1)] + [(tp, T - tp) for T in (tc - 1, tc, tc + 1, 2 * tc + 3) for tp in (1, 3)]


R_EDGES = [(n_tx, n_rx, P, tp, td)
           for (n_tx, n_rx, P), tc in (((4, 1, 1), 16), ((4, 4, 69), 32), ((4, 2, 131), 8),
                                       ((8, 1, 1), 16))
           for tp, td in _t_edges(tc)]
# the B^H kernels at their smallest P of the grid (and rhs_dma_kernel's last P before
# rhs_lds_kernel): the last chunk partial by 1, full, over by 1, and two chunks + 1
RHS_EDGES = [(n_tx, n_rx, P, TP, td)
             for (n_tx, n_rx, P), tds in (((4, 1, 1), (1, 15, 16, 17, 33)),
                                          ((2, 2, 124), (1, 15, 16, 17, 33)),
                                          ((2, 2, 125), (1, 15, 16, 17, 33)),
                                          ((1, 3, 129), (1, 3, 4, 5, 9)),
                                          ((1, 2, 512), (1, 3, 4, 5, 9)))
             for td in tds]


def test_edge_lists_fit_the_chunks():
    for n_tx, n_rx, P, tp, td in R_EDGES:
        assert tp >= 1 and td >= 1
    assert sorted({tp + td for n_tx, _, P, tp, td in R_EDGES if (n_tx, P) == (4, 131)}) == \
        [2, 7, 8, 9, 19]
    for n_tx, n_rx, P, tp, td in RHS_EDGES:
        tcr = rhs_route(n_tx, n_rx, P)[1]
        assert td in (1, tcr - 1, tcr, tcr + 1, 2 * tcr + 1)


@pytest.mark.parametrize("n_tx,n_rx,P,T_p,T_d", R_EDGES + RHS_EDGES)
def test_symbol_count_edges(sbce, n_tx, n_rx, P, T_p, T_d):
    b, ref = problem(3, n_tx, n_rx, P, T_p, T_d)
    check_build(b, ref, run(sbce, b), "edge " + label_of(n_tx, n_rx, P, T_p, T_d))


# ------------------------------------------------------------------ row 7: the gated rebuild
@pytest.mark.parametrize("n_tx,n_rx,P", [(4, 2, 21), (8, 3, 10), (4, 8, 128)])
def test_gated_rebuild(sbce, n_tx, n_rx, P):
    """One trial of three whose u_p is no Kronecker product: flagged, rebuilt by the VALU
    kernel from u_p itself, and every trial (the MFMA-built two as well) under the bound."""
    b, ref = problem(3, n_tx, n_rx, P, TP, TD, broken=1)
    out = run(sbce, b)
    pilot = [bool(v & sbce._lib.SBCE_STATUS_PILOT) for v in out[3]]
    assert pilot == [False, True, False]
    check_build(b, ref, out, "row 7 gated " + label_of(n_tx, n_rx, P))


# ------------------------------------------------------------------ row 8: L <= 64, one workgroup
SMALL = [(5, 2, 12), (6, 8, 10), (7, 3, 9), (5, 1, 1), (3, 4, 16), (1, 2, 10), (2, 8, 16)]


@pytest.mark.parametrize("n_tx,n_rx,P", SMALL)
def test_small_build_arms(sbce, n_tx, n_rx, P):
    """The default build and the SBCE_MSTEP_SMALL arms 0 (the batched path), 1 (the round-5
    MFMA kernel where it applies) and v (the VALU build), each against the reference."""
    assert r_route(n_tx, P) == "small"
    b, ref = problem(3, n_tx, n_rx, P, TP, TD)
    check_build(b, ref, run(sbce, b), f"row 8 small default ({n_tx},{n_rx},{P})")
    for arm in ("0", "1", "v"):
        check_build(b, ref, run(sbce, b, env=dict(SBCE_MSTEP_SMALL=arm)),
                    f"row 8 small arm {arm} ({n_tx},{n_rx},{P})")


# ------------------------------------------------------------------ workspace independence
@pytest.mark.parametrize("row,n_tx,n_rx,P,broken", [
    (1, 4, 2, 22, None), (2, 4, 3, 100, None), (3, 4, 2, 131, None), (4, 8, 3, 11, None),
    (5, 3, 6, 22, None), (6, 6, 5, 11, None), (7, 4, 2, 21, 1), (8, 5, 2, 12, None)])
def test_workspace_independence(sbce, row, n_tx, n_rx, P, broken):
    """R, rhs, theta and status are bitwise the same whatever the workspace held."""
    b, _ = problem(3, n_tx, n_rx, P, TP, TD, broken)
    o0, o1 = (run(sbce, b, ws_fill=f) for f in (0x00, 0xFF))
    for x, y, name in zip(o0, o1, ("theta", "R", "rhs", "status")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (row, name)


# ------------------------------------------------------------------ solve at well-posed shapes
@pytest.mark.parametrize("n_tx,n_rx,P,T_p,T_d", [
    (7, 3, 9, 4, 20), (5, 2, 12, 3, 30), (6, 8, 10, 5, 25), (5, 4, 20, 5, 45), (6, 5, 30, 6, 60),
    (7, 2, 73, 7, 120), (5, 3, 103, 8, 150), (6, 2, 86, 6, 130), (4, 3, 100, 16, 160),
    (8, 4, 64, 16, 100), (4, 2, 1, 2, 5)])
def test_solve_at_well_posed_shapes(sbce, n_tx, n_rx, P, T_p, T_d):
    """theta against numpy's solve of the REFERENCE system (not of what the device built), at
    the bars test_gpu_em.py holds; no trial flagged."""
    b, ref = problem(3, n_tx, n_rx, P, T_p, T_d)
    out = run(sbce, b)
    check_build(b, ref, out, "solve " + label_of(n_tx, n_rx, P, T_p, T_d))
    th, _, _, st = out
    assert not st.any(), st
    for i, (R0, rhs0, _, _) in enumerate(ref):
        R64, rhs64 = R0.astype(np.complex128), rhs0.astype(np.complex128)
        cond = np.linalg.cond(R64)
        assert cond < 1e4, "the shape must be well posed: change the seed, not the cap"
        want = np.conj(np.linalg.solve(R64, rhs64)).reshape(-1)
        err = rel(th[i], want)
        print(f"[mstep-build] solve ({n_tx},{n_rx},{P}) trial {i}: cond {cond:.1f} rel {err:.2e}")
        assert err < (max(1e-12, 1e-15 * cond) if P * n_tx <= 512 else 1e-9), cond


# ------------------------------------------------------------------ chains at n_tx = 5, 6
@pytest.mark.parametrize("shape", [
    # (n_tx, n_rx, N, T_p, T_d, M, r)
    (5, 6, 4, 30, 48, 4, 2),          # L = 25: the one-workgroup M-step
    (6, 6, 14, 48, 120, 4, 2),        # L = 90: rbuild_wide_kernel<6> + the batched Cholesky
])
def test_pm_soft_full_em_nt5_nt6_vs_oracle(sbce, shape):
    """Three PM-soft EM iterations on the device vs oracle.pm.em_pm at n_tx the suite ran no
    chain at (as test_pm_soft_full_em_cfg2_geometry_vs_oracle does at n_tx = 8)."""
    from oracle.pm import em_pm
    n_tx, n_rx, N, T_p, T_d, M, r = shape
    varn, itera = 0.05, 3
    b = sbce.signal_model.synthetic_batch(3, n_tx, n_rx, N, T_p, T_d, M, varn, seed=9)
    res = sbce.em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], varn, itera,
                        b["theta0"], mode="pm_soft", partition_r=r)
    assert not res["status"].any()
    for i in range(3):
        th = em_pm(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, varn, itera,
                   b["theta0"][i], n_tx, n_rx, r, b["cons"], soft=True)
        assert rel(res["theta"][i], th) < 1e-9
