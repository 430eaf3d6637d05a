"""GPU tier: the exact E-step (SBCE_ESTEP_SOFT / SBCE_ESTEP_HARD) on tables that are not the
reference modem's square QAM, at n_tx = 3 with the sphere pass, on the MFMA geometry classes and
n_rx values no other test launches, and on exact ties -- against the extended-precision
restatement of tests/estep_ref.py (any table, itertools.product order, first minimum).

Coverage (C rows; counters of the A/B build under SBCE_ESTEP_COUNT=1: sph = sbce_debug_estep_sphere
[enumerated, listed, single path], pair = sbce_debug_estep_pair, mfma = sbce_debug_estep_mfma):

row  shape x B                tables                         kernels                               proof
 1   (2, 2|5|6|7, 5, 7) x 3   qam16_rot psk16 cross32 apsk64 estep_tree_kernel<2, NR>; soft:       soft: pair == 0, and mfma > 0
                              (grid_build: K = 0 for all)    estep_fact2 / soft2_kernel<NR> push   exactly when sph[2] < symbols;
                                                             every symbol to the sweep's list,     hard: pair == symbols - sph[2]
                                                             estep_bounds_kernel<2, NR>,
                                                             estep_mfma_kernel<2, NR, SOFT, 1>
                                                             (M = 64: TU = 4); hard:
                                                             estep_hard2_kernel<NR> scans all M
 2   (2, 3|6|7, 5, 7) x 3     qam16_perm qam16_uneven qam64  fact2 tables (wide), soft2 box        soft: pair > 0 at -5 dB;
                              (K = 4, 4, 8)                  (narrow), hard2 per-axis search       hard: pair == symbols - sph[2]
 3   (2, 2, 4, 7) x 3         bpsk psk8                      estep_kernel<2, 2, 1, *> (JA < 16)    mfma == 0, sph == 0, pair == 0
 4   (3, 3..8, 3, 7) x 3      qam16; psk16, qam16_uneven     estep_tree_kernel<3, NR>,             sum(sph) == symbols; mfma > 0
                              at n_rx = 3, 7                 estep_bfs_kernel<3, 1|2>,             exactly when sph[1] > 0
                                                             estep_bounds_kernel<3, NR>,
                                                             estep_mfma_kernel<3, NR, *, 1>
 5   (3, 3|2, 2, 5) x 1       qam64 cross32                  n_rx = 3: as row 4 with TU = 4        n_rx = 2: sum(sph) == 0 and
                                                             (M = 64, chunk 64) / TU = 1 (M = 32,  mfma > 0; n_rx = 3: as row 4
                                                             chunk 32); n_rx = 2:
                                                             estep_prep_kernel<3, 2> + the
                                                             unlisted sweep
 6   (4, 4|6|7, 2, 7) x 3     psk8                           tree / bfs<4, *> / bounds<4, NR>,     as row 4
                                                             estep_mfma_kernel<4, NR, *, 4>
                                                             (generic body, row-tile bounds)
 7   (4, 4, 2, 5) x 1         cross32                        as row 6, JA = JB = 1024, chunk 256   as row 4; the 0 dB case
     at 20 dB; (4, 4, 2, 3)                                                                        lists symbols on the
     x 1 at 0 dB                                                                                   default route (sph[1] > 0)
 8   (4, 6|7, 3, 7) x 3       qam16 qam16_perm psk16         estep_mfma_kernel<4, NR, *, 4, true>  soft: pair > 0 at -5 dB,
                                                             (V16), estep_pair_kernel<NR>          pair == 0 with SBCE_ESTEP_PAIR=0

Second opinions from the device, each held to the restatement and to the default arm: the VALU
kernel (SBCE_ESTEP_IMPL=valu, rows 1, 2, 4), the enumeration instead of the pair passes
(SBCE_ESTEP_PAIR=0, rows 1, 2, 8), and, for the rows with n_tx >= 3 and the sphere pass, a path
list of one (SBCE_SPHERE_BUDGET=1: every symbol with a second path is listed for the bounds pass
and the listed sweep) and no sphere pass (SBCE_ESTEP_SPHERE=0: estep_prep_kernel<NT, NR> and the
unlisted sweep weigh every symbol; sph == 0, mfma > 0).  Which symbols the default switches list
depends on the posteriors' width -- row 7's 20 dB posteriors are one-hot and mostly enumerated;
its added 0 dB case has wide ones, listed on the default route too --
so these two arms are what puts EVERY case's symbols through the sweep instantiation of its row.

What the counters cannot tell: TU = 1 from TU = 4 and the V16 body from the generic one (mfma
counts the MFMAs of whichever sweep ran; dispatch_mfma_mode picks by (n_tx, M, chunk) alone, so
the shape fixes the instantiation); and in pair mode at n_tx = 2 the enumeration is not launched,
so sph[0] and sph[1] stay 0 and the listed symbols are symbols - sph[2] - pair.
Row 8, psk16: both run.  dispatch_mfma_mode takes the V16 body for every (n_tx = 4, M = 16) table
and estep_pair_supported asks for (n_tx = 4, M = 16, 4 <= n_rx <= 8, soft) only;
estep_pair_kernel builds its six 16 x 16 tables over table INDICES and needs no grid.
Row 1, hard mode: estep_hard2_kernel does not hand over on K = 0 (it scans all M points per
lane), so there the pair counter is NOT 0.
The `nf == 64` flush of the fact2 / soft2 hand-over needs one wave to fail 64 symbols (more than
500k symbols a launch): only the final flush runs here.

Conditions on the inputs (asserted on the host before the first device call): every symbol's
reference gap (d_second - d_min) / d_min exceeds 1e-9 for the hard decisions of C; cond(R) <
1e12 for the full chain of E.  The seeds were chosen on the host to meet them."""
import ctypes

import numpy as np
import pytest

import estep_ref as er

pytestmark = pytest.mark.gpu

SOFT_TOL = 1e-11          # x max|c|^2: test_gpu_em.py test_estep_moments_vs_oracle
HERM_TOL = 1e-12
HARD_S_TOL = 1e-13
GAP_MIN = 1e-9
THETA_TOL = 1e-10         # test_gpu_em.py


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """torch must bring the HIP runtime up before the library's diagnostic entry points do."""
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


def _cases():
    out = []

    def add(row, n_tx, n_rx, N, T_d, B, tables, snrs):
        for tab in tables:
            for snr in snrs:
                out.append((row, n_tx, n_rx, N, T_d, B, tab, snr))
    for n_rx in (2, 5, 6, 7):
        add(1, 2, n_rx, 5, 7, 3, ("qam16_rot", "psk16", "cross32", "apsk64"), (-5, 10, 30))
    for n_rx in (3, 6, 7):
        add(2, 2, n_rx, 5, 7, 3, ("qam16_perm", "qam16_uneven", "qam64"), (-5, 10, 30))
    add(3, 2, 2, 4, 7, 3, ("bpsk", "psk8"), (0, 20))
    for n_rx in (3, 4, 5, 6, 7, 8):
        tabs = ("qam16", "psk16", "qam16_uneven") if n_rx in (3, 7) else ("qam16",)
        add(4, 3, n_rx, 3, 7, 3, tabs, (0, 15, 30))
    for n_rx in (3, 2):
        add(5, 3, n_rx, 2, 5, 1, ("qam64", "cross32"), (10, 30))
    for n_rx in (4, 6, 7):
        add(6, 4, n_rx, 2, 7, 3, ("psk8",), (0, 20))
    add(7, 4, 4, 2, 5, 1, ("cross32",), (20,))
    for n_rx in (6, 7):
        add(8, 4, n_rx, 3, 7, 3, ("qam16", "qam16_perm", "psk16"), (-5, 20))
    # row 7 again where the soft sum over the 2^20 hypotheses is a sum: at 20 dB its posteriors are
    # one-hot.  Three symbols (each costs the restatement two passes over 2^20 hypotheses); last
    # in the list, so that the cases above keep their seeds
    add(7, 4, 4, 2, 3, 1, ("cross32",), (0,))
    return out


CASES = _cases()
# the batch generator's seed per case: its position in CASES + 1, except where that draw leaves a
# symbol with a reference gap below GAP_MIN (none did)
SEEDS = {}
_cache = {}


def _cid(c):
    row, n_tx, n_rx, N, T_d, B, tab, snr = c
    return f"r{row}-{n_tx}x{n_rx}-{tab}-{snr}dB"


def case_inputs(c):
    """The case's batch and the restatement's moments at both channel arguments; asserts the gap
    condition.  Host only (the seed search runs it without a device)."""
    if c not in _cache:
        row, n_tx, n_rx, N, T_d, B, tab, snr = c
        cons = er.table(tab)
        b = er.synthetic_batch(cons, B, n_tx, n_rx, N, T_d, snr,
                               seed=SEEDS.get(_cid(c), CASES.index(c) + 1))
        refs = {k: er.batch_moments(b["theta_" + k], b["y_d"], b["psi_d"], cons, b["varn"], n_tx)
                for k in ("wide", "narrow")}
        for k, r in refs.items():
            assert r["gap"].min() > GAP_MIN, (_cid(c), k, r["gap"].min())
            for v in r.values():
                v.setflags(write=False)
        _cache[c] = (b, refs)
    return _cache[c]


def _run(sbce, b, th, mode, **env):
    """One device E-step on the A/B build with the counters read: (m, S, dict(sph, pair, mfma))."""
    lib = sbce._lib.load_ab()
    with sbce._lib.debug_env(SBCE_ESTEP_COUNT="1", **env):
        lib.sbce_debug_estep_sphere(None, 1)
        lib.sbce_debug_estep_pair(None, 1)
        lib.sbce_debug_estep_mfma(None, 1)
        m, S = sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], th, b["varn"], b["n_tx"], mode)
        sph = (ctypes.c_ulonglong * 3)()
        lib.sbce_debug_estep_sphere(sph, 0)
        pair, mfma = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        lib.sbce_debug_estep_pair(ctypes.byref(pair), 0)
        lib.sbce_debug_estep_mfma(ctypes.byref(mfma), 0)
    return m, S, dict(sph=[int(v) for v in sph], pair=int(pair.value), mfma=int(mfma.value))


def _exact_products(cons):
    """Every x_r x_i of the table is exact in binary64: levels that are multiples of 1/2."""
    v = np.concatenate([cons.real, cons.imag]) * 2
    return bool(np.all(v == np.round(v)))


def _soft_errors(m, S, ref, scale):
    return np.abs(m - ref["m"]).max() / scale, np.abs(S - ref["S"]).max() / scale


def _assert_soft(m, S, ref, scale, tag, exact_products):
    em, es = _soft_errors(m, S, ref, scale)
    print(f"estep_tables {tag} soft: |m - m_ref| {em:.2e} |S - S_ref| {es:.2e} (x max|c|^2)")
    assert np.all(np.isfinite(m.view(float))) and np.all(np.isfinite(S.view(float))), tag
    assert em < SOFT_TOL and es < SOFT_TOL, (tag, em, es)
    assert np.abs(S - np.conj(np.swapaxes(S, -1, -2))).max() < HERM_TOL * scale, tag
    # the diagonal is real: exactly where x_r x_i is exact in binary64 (integer and half-integer
    # levels), else to the rounding of one |x|^2 (x conj(x) contracted to an fma leaves up to an
    # ulp of x_r x_i in the imaginary part, and a weighted mean of such terms is no larger)
    dim = np.abs(np.diagonal(S, axis1=-2, axis2=-1).imag).max()
    assert dim <= (0.0 if exact_products else 4 * np.finfo(float).eps * scale), (tag, dim)


def _assert_hard(m, S, ref, tag):
    assert np.array_equal(m, ref["mh"]), tag
    assert np.abs(S - ref["Sh"]).max() < HARD_S_TOL, (tag, np.abs(S - ref["Sh"]).max())


def _assert_route(c, kind, mode, cnt, nsym):
    """The route of the case (module docstring) from the counters of the default switches."""
    row, n_tx, n_rx, N, T_d, B, tab, snr = c
    sph, pair, mfma = cnt["sph"], cnt["pair"], cnt["mfma"]
    low = snr == min(cc[7] for cc in CASES if cc[0] == row)
    tag = (_cid(c), kind, mode, cnt)
    if row in (1, 2):
        # pair mode at n_tx = 2: no enumeration, every symbol is single-path, the pair passes' or
        # (soft only) the sweep's
        assert sph[0] == 0 and sph[1] == 0 and sph[2] <= nsym, tag
        K = er.grid_k(er.table(tab))
        assert (K == 0) == (row == 1), tag
        if mode == "hard":
            assert pair == nsym - sph[2], tag               # hard2 resolves every symbol it gets
        elif row == 1:
            assert pair == 0, tag                           # K = 0: fact2 and soft2 hand over
            assert (mfma > 0) == (sph[2] < nsym), tag       # ... to the sweep, whatever is left
            if low:
                # varn^2 is 10 E_s^2: no symbol's sphere holds one hypothesis
                assert sph[2] < nsym, tag
        else:
            assert pair <= nsym - sph[2], tag
            if low:
                assert pair > 0, tag
            if pair < nsym - sph[2]:                        # a symbol out of the tables' range
                assert mfma > 0, tag
    elif row == 3:
        assert sph == [0, 0, 0] and pair == 0 and mfma == 0, tag
    elif row == 5 and n_rx < n_tx:
        assert sph == [0, 0, 0] and pair == 0 and mfma > 0, tag
    else:
        assert sum(sph) == nsym, tag
        assert (mfma > 0) == (sph[1] - pair > 0), tag
        if row == 8:
            if mode == "soft" and low and kind == "wide":
                assert pair > 0, tag
            if mode == "hard":
                assert pair == 0, tag
        else:
            assert pair == 0, tag
        if row == 4 and snr == 30 and kind == "narrow":
            assert sph[0] + sph[2] > 0, tag
        if low and kind == "wide" and mode == "soft" and row in (4, 5, 6, 7):
            # the sphere radius 50 varn^2 is several times ||H (x - x')||^2 of neighbouring
            # hypotheses: more paths than the enumeration's list holds (128 a level), so symbols
            # are listed and the sweep runs.  (Row 7 at 20 dB: the radius is small -- there the
            # forced arms of the test are what puts the 2^20 hypotheses through the sweep.)
            assert sph[1] > 0, tag


@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_estep_tables_vs_restatement(sbce, c):
    """Rows 1-8 of the module docstring: soft moments and hard decisions against the restatement
    at wide and narrow posteriors, the route from the counters, and the second opinions from
    the device (VALU kernel, no pair passes, a path list of one, no sphere pass)."""
    row, n_tx, n_rx, N, T_d, B, tab, snr = c
    b, refs = case_inputs(c)
    scale = np.abs(b["cons"]).max() ** 2
    nsym = B * T_d
    arms = [{}]
    if row in (1, 2, 4):
        arms.append(dict(SBCE_ESTEP_IMPL="valu"))
    if row in (1, 2, 8):
        arms.append(dict(SBCE_ESTEP_PAIR="0"))
    if row >= 4 and n_rx >= n_tx:
        # whatever the posteriors' width routes where: a path list of one lists every symbol with
        # a second path for the bounds pass and the listed sweep, and without the sphere pass
        # the preparation pass and the unlisted sweep weigh every symbol
        arms.append(dict(SBCE_SPHERE_BUDGET="1"))
        arms.append(dict(SBCE_ESTEP_SPHERE="0"))
    for kind in ("wide", "narrow"):
        th, ref = b["theta_" + kind], refs[kind]
        out = {}
        for i, env in enumerate(arms):
            for mode in ("soft", "hard"):
                out[i, mode] = _run(sbce, b, th, mode, **env)
                print(f"estep_tables {_cid(c)} {kind} {mode} {env}: {out[i, mode][2]}")
        # the product library: the same kernels without the switches
        mp, Sp = sbce.estep_batch(b["y_d"], b["psi_d"], b["cons"], th, b["varn"], n_tx)
        assert np.array_equal(mp, out[0, "soft"][0]) and np.array_equal(Sp, out[0, "soft"][1])
        for i, env in enumerate(arms):
            tag = f"{_cid(c)} {kind} {env}"
            m, S, cnt = out[i, "soft"]
            _assert_soft(m, S, ref, scale, tag, _exact_products(b["cons"]))
            mh, Sh, cnth = out[i, "hard"]
            _assert_hard(mh, Sh, ref, tag)
            if "SBCE_ESTEP_IMPL" in env:
                assert cnt["mfma"] == 0 and cnth["mfma"] == 0 and cnt["pair"] == 0, tag
            if "SBCE_ESTEP_PAIR" in env:
                assert cnt["pair"] == 0 and cnth["pair"] == 0, tag
                assert sum(cnt["sph"]) == nsym and sum(cnth["sph"]) == nsym, tag
            if "SBCE_SPHERE_BUDGET" in env:
                for k, d in ((cnt, out[0, "soft"][2]), (cnth, out[0, "hard"][2])):
                    assert sum(k["sph"]) == nsym and k["sph"][1] >= d["sph"][1], tag
                    assert (k["mfma"] > 0) == (k["sph"][1] - k["pair"] > 0), tag
            if "SBCE_ESTEP_SPHERE" in env:
                for k in (cnt, cnth):
                    assert k["sph"] == [0, 0, 0] and k["pair"] == 0 and k["mfma"] > 0, tag
            if i:
                assert np.abs(m - out[0, "soft"][0]).max() < SOFT_TOL * scale, tag
                assert np.abs(S - out[0, "soft"][1]).max() < SOFT_TOL * scale, tag
                assert np.array_equal(mh, out[0, "hard"][0]), tag
        _assert_route(c, kind, "soft", out[0, "soft"][2], nsym)
        _assert_route(c, kind, "hard", out[0, "hard"][2], nsym)


# ------------------------------------------------------------------ D: ties, degenerate channels
TIE_SHAPES = [(2, 3), (3, 4), (4, 4)]


def _tie_inputs(n_tx, n_rx, tab, kind):
    key = ("tie", n_tx, n_rx, tab, kind)
    if key not in _cache:
        cons = er.table(tab)
        b = er.synthetic_batch(cons, 3, n_tx, n_rx, 2, 7, 10, seed=17 + n_tx)
        b["varn"] = 0.3
        if kind == "zero":
            th = np.zeros_like(b["h"])
        else:
            th = b["h"].reshape(3, 3, n_tx, n_rx).copy()          # [trial, p, a, r]
            th[:, :, 1, :] = 0.0
            th = th.reshape(3, -1)
        ref = er.batch_moments(th, b["y_d"], b["psi_d"], cons, 0.3, n_tx)
        assert np.all(ref["gap"] == 0)                             # these ARE the tie cases
        assert np.all(ref["mh"][..., 1] == cons[0])
        if kind == "column":
            # the other streams' decisions: the problem without stream 1 has no tie
            keep = [a for a in range(n_tx) if a != 1]
            thr = th.reshape(3, 3, n_tx, n_rx)[:, :, keep, :].reshape(3, -1)
            red = er.batch_moments(thr, b["y_d"], b["psi_d"], cons, 0.3, n_tx - 1)
            assert red["gap"].min() > GAP_MIN
            assert np.array_equal(red["mh"], ref["mh"][..., keep])
        _cache[key] = (b, th, ref)
    return _cache[key]


@pytest.mark.parametrize("kind", ["zero", "column"])
@pytest.mark.parametrize("tab", ["qam16", "psk16"])
@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_and_degenerate_channels(sbce, shape, tab, kind):
    """theta = 0 (H_t = 0: all J distances equal) and one stream's channel column exactly zero
    (a singular Gram matrix under the sphere pass; M^(n_tx - 1) classes of M tied hypotheses),
    21 symbols, varn = 0.3.  Soft: the restatement's moments (theta = 0: the uniform posterior,
    m = mean(cons), S_aa = mean|c|^2, S_ab = |mean(cons)|^2).  Hard: the first minimum in
    product order -- cons[0] on every tied stream, as np.argmin and the reference's
    zero-initialised scripts have it."""
    n_tx, n_rx = shape
    b, th, ref = _tie_inputs(n_tx, n_rx, tab, kind)
    cons = b["cons"]
    scale = np.abs(cons).max() ** 2
    if kind == "zero":
        mu, e = cons.mean(), np.mean(np.abs(cons) ** 2)
        S0 = np.full((n_tx, n_tx), abs(mu) ** 2, dtype=complex) + (e - abs(mu) ** 2) * np.eye(n_tx)
        assert np.abs(ref["m"] - mu).max() < 1e-15 and np.abs(ref["S"] - S0).max() < 1e-14
        assert np.all(ref["mh"] == cons[0])
    # the default route (n_tx = 2: hard2's scan, fact2, soft2's `deg` branch; above: the tree pass
    # lists a symbol with a ridge-only pivot for the sweep), the VALU kernel, and every other
    # writer the switches can send a tied symbol to.  SBCE_ESTEP_PAIR=0 at n_tx = 2 is the arm
    # that found estep_bfs_kernel<2, 2> ordering exact ties by the rounding of its path bounds
    # (theta = 0 and the zero column decided a later table entry than cons[0]) before the tree
    # pass sent such symbols to the sweep.
    arms = [{}, dict(SBCE_ESTEP_IMPL="valu")]
    arms += ([dict(SBCE_ESTEP_PAIR="0")] if n_tx == 2 else
             [dict(SBCE_SPHERE_BUDGET="1"), dict(SBCE_ESTEP_SPHERE="0")])
    for env in arms:
        tag = f"{n_tx}x{n_rx} {tab} {kind} {env}"
        m, S, cnt = _run(sbce, b, th, "soft", **env)
        mh, Sh, cnth = _run(sbce, b, th, "hard", **env)
        print(f"estep_tables tie {tag}: soft {cnt} hard {cnth}")
        _assert_soft(m, S, ref, scale, tag, _exact_products(cons))
        assert np.all(np.isfinite(mh.view(float))) and np.all(np.isfinite(Sh.view(float))), tag
        _assert_hard(mh, Sh, ref, tag)


# ------------------------------------------------------------------ E: other modes, full chain
@pytest.mark.parametrize("tab", ["psk16", "qam16_rot", "qam16_uneven"])
def test_detector_and_pm_modes_on_other_tables(sbce, tab):
    """ZF / MMSE / PM / PM-soft (partition_r = 1) at (2, 3, N = 4, T_d = 9) x 2: estep_pm.hip's
    nearest_point on a table that is no grid (nearest_scan: psk16, qam16_rot) and on a grid with
    unequal, off-centre levels (the per-axis search: qam16_uneven), against the oracles, with the
    tolerances of test_detector_estep_vs_oracle and test_pm_estep_moments_vs_oracle."""
    from oracle.detectors import detector_moments
    from oracle.pm import pm_moments
    cons = er.table(tab)
    b = er.synthetic_batch(cons, 2, 2, 3, 4, 9, 15, seed=21)
    scale = np.abs(cons).max() ** 2
    for kind in ("wide", "narrow"):
        th = b["theta_" + kind]
        for mode in ("zf", "mmse"):
            m, S = sbce.estep_batch(b["y_d"], b["psi_d"], cons, th, b["varn"], 2, mode)
            for i in range(2):
                m0, S0 = detector_moments(th[i], b["y_d"][i], b["psi_d"][i].T, None, b["varn"],
                                          2, 3, mode, cons=cons)
                assert np.array_equal(m[i], m0), (tab, kind, mode)
                assert np.allclose(S[i], S0, rtol=0, atol=1e-12), (tab, kind, mode)
        for mode, soft in (("pm", False), ("pm_soft", True)):
            m, S = sbce.estep_batch(b["y_d"], b["psi_d"], cons, th, b["varn"], 2, mode, 1)
            nlist = 1 if soft else cons.size
            for i in range(2):
                m0, S0 = pm_moments(th[i], b["y_d"][i], b["psi_d"][i].T, cons, 2, 3, 1, b["varn"],
                                    soft)
                assert np.abs(m[i] - m0).max() < 1e-11 * scale * nlist, (tab, kind, mode)
                assert np.abs(S[i] - S0).max() < 1e-11 * scale * nlist, (tab, kind, mode)


def _chain_inputs(n_tx, n_rx, N, tab, seed):
    """The full-chain batch and the oracle's two iterations per trial and mode, with cond(R) of
    every oracle M-step asserted below 1e12 (host only)."""
    from oracle.em_reduced import estep_moments, mstep_build, mstep_solve, aps_from_cons
    key = ("chain", n_tx, n_rx, N, tab, seed)
    if key not in _cache:
        cons = er.table(tab)
        b = er.synthetic_batch(cons, 2, n_tx, n_rx, N, 21, 15, seed=seed, T_p=12)
        aps = aps_from_cons(cons, n_tx)
        ref = {}
        for mode in ("soft", "hard"):
            ths = []
            for i in range(2):
                th = b["theta0"][i]
                for _ in range(2):
                    m, S, _, _ = estep_moments(th, b["y_d"][i], b["psi_d"][i].T, aps, b["varn"], mode)
                    R, rhs = mstep_build(b["u_p"][i], b["y_p"][i], b["psi_d"][i].T, b["y_d"][i], m, S)
                    assert np.linalg.cond(R) < 1e12, "the shape must be well posed"
                    th = mstep_solve(R, rhs)
                ths.append(th)
            ref[mode] = np.stack(ths)
        _cache[key] = (b, aps, ref)
    return _cache[key]


CHAINS = [(2, 2, 5, "psk16", 31), (3, 3, 3, "qam16", 32)]


@pytest.mark.parametrize("shape", CHAINS, ids=lambda s: f"{s[0]}x{s[1]}-{s[3]}")
def test_full_chain_two_iterations_vs_oracle(sbce, shape):
    """Two EM iterations (sbce_em, soft and hard) at (2, 2, N = 5) on psk16 -- no grid: the sweep
    weighs what the n_tx = 2 passes hand over -- and at (3, 3, N = 3) on 16-QAM (tree pass,
    enumeration, bounds and sweep at n_tx = 3), T_p = 12, T_d = 21, against oracle.em_reduced."""
    from oracle.em_reduced import em_reduced
    from conftest import rel
    n_tx, n_rx, N, tab, seed = shape
    b, aps, ref = _chain_inputs(n_tx, n_rx, N, tab, seed)
    for mode in ("soft", "hard"):
        r = sbce.em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], b["varn"], 2,
                          b["theta0"], mode=mode)
        assert np.all(r["status"] == 0) and np.all(r["iters_done"] == 2)
        for i in range(2):
            th0 = em_reduced(b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, aps,
                             b["varn"], 2, b["theta0"][i], mode)
            assert np.array_equal(th0, ref[mode][i])
            e = rel(r["theta"][i], th0)
            print(f"estep_tables chain {n_tx}x{n_rx} {tab} {mode} trial {i}: rel err {e:.2e}")
            assert e < THETA_TOL, (mode, i, e)
