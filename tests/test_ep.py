"""CPU tier of expectation propagation (SBCE_ESTEP_EP, SBCE_LINEAR_EP): the guards the GPU parity
tests (tests/test_gpu_estep_ep.py) rely on, the bound's constant measured against a 50-digit copy
of the restatement (tests/ep_oracle.py), the identity that ties one pass to the soft MMSE
restatement, and the two conditions that make EP worth having: fewer symbol errors than MMSE at
8 x 8, and a better channel estimate from the EM chain."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ep_oracle as ep
import linear_em_oracle as eo
import linear_oracle as lo

HEADER = os.path.join(ROOT, "include", "sbce.h")


# ------------------------------------------------------------------ 1. guards of the parity cases
@pytest.mark.parametrize("si,vi", ep.CASES)
def test_parity_cases_cannot_flip_a_branch(si, vi):
    """p = 5: no failed pivot; no update within 1e-6 (relative) of r' = 0 and no variance within
    1e-3 (relative) of its floor, so rounding decides neither branch; each stream's two nearest
    table points a relative 1e-6 apart, so idx_hat is pinned."""
    o = ep.ref(si, vi)
    print(f"{ep.SHAPES[si]} varn {ep.VARNS[vi]}: max cond(A) {o['kappa'].max():.3g}, margin_r "
          f"{o['margin_r'].min():.3g}, margin_v {o['margin_v'].min():.3g}, gap {o['gap'].min():.3g}, "
          f"kept {o['kept'].sum()}, clamped {o['clamped'].sum()}")
    assert not o["fail"].any() and not o["status"].any()
    assert o["margin_r"].min() >= 1e-6
    assert o["margin_v"].min() >= 1e-3
    assert o["gap"].min() >= 1e-6
    assert np.all(np.isfinite(o["nu"])) and np.all(o["nu"] > 0)
    assert np.allclose(o["post"].sum(axis=-1), 1.0, atol=1e-12)


def test_parity_cases_take_both_branches():
    """The set exercises the kept update (r' <= 0) and the variance floor, and cond(A) grows past
    1e6 where the floor makes r large on decided streams."""
    refs = [ep.ref(si, vi) for si, vi in ep.CASES]
    kept = sum(bool(o["kept"].sum()) for o in refs)
    clamped = sum(bool(o["clamped"].sum()) for o in refs)
    kappa = max(o["kappa"].max() for o in refs)
    print(f"kept in {kept} of {len(refs)} cases, clamped in {clamped}, max cond(A) {kappa:.3g}")
    assert kept >= 8 and clamped >= 8 and kappa >= 1e6
    assert ep.SHAPES is lo.SHAPES and ep.VARNS is lo.VARNS
    assert [s != t for s, t in zip(ep.SEEDS, lo.SEEDS)] == [False] * 4 + [True] + [False] * 3


@pytest.mark.parametrize("passes", [1, 2, 16])
def test_pass_sweep_cases_hold_the_guards(passes):
    """(8,8,5,24,16) at varn 1.0, the case the GPU tier sweeps the pass count on."""
    o = ep.ref(5, 1, passes)
    assert not o["fail"].any()
    assert o["margin_r"].min() >= 1e-6 and o["margin_v"].min() >= 1e-3 and o["gap"].min() >= 1e-6


def test_multi_workgroup_case_fails_where_planted():
    """T_d = 70: exactly trial 1's symbols from DEFECT_T0 on lose a pivot (its varn = 1e-8 puts r
    below the pivot rule), all of them in the trial's second and third workgroup; the other
    symbols hold the guards."""
    o = ep.chunk_ref()
    want = np.zeros((3, 70), bool)
    want[1, lo.DEFECT_T0:] = True
    assert np.array_equal(o["fail"], want) and list(o["status"]) == [0, lo.NONHPD, 0]
    ok = ~o["fail"]
    assert o["margin_r"][ok].min() >= 1e-6 and o["margin_v"][ok].min() >= 1e-3
    assert o["gap"][ok].min() >= 1e-6 and lo.DEFECT_T0 >= 32


# ------------------------------------------------------------------ 2. the constant
def test_constant_against_extended_precision():
    """r over all parity cases, overall and output by output; C_EP = 16 max(r, 1) and the
    per-output constants 16 max(r_k, 1) are what ep_oracle holds."""
    worst, where, by = 0.0, None, {}
    for si, vi in ep.CASES:
        c, o = ep.case(si, vi), ep.ref(si, vi)
        m = ep.ep_ref_mp(c["y"], c["psi"], c["cons"], c["theta"], ep.VARNS[vi] ** 2, c["n_tx"],
                         ep.PASSES, lo.default_es(c["cons"]), c["labels"])
        for k, v in lo.ratios(m, o, c["cons"]).items():
            by[k] = max(by.get(k, 0.0), v)
            if v > worst:
                worst, where = v, (ep.SHAPES[si], ep.VARNS[vi], k)
    print(f"r = {worst:.3f} at {where}; C_EP = {ep.C_EP}; by output "
          + ", ".join(f"{k} {v:.4g}" for k, v in by.items()))
    assert set(by) == set(ep.R_BY_OUTPUT)
    for k, v in by.items():
        assert 0.9 * ep.R_BY_OUTPUT[k] <= v <= ep.R_BY_OUTPUT[k], (k, v)
        assert ep.C_BY_OUTPUT[k] == 16.0 * max(ep.R_BY_OUTPUT[k], 1.0) <= ep.C_EP
    assert worst <= ep.R_MEASURED
    assert worst >= 0.9 * ep.R_MEASURED          # the recorded figure is the measured one
    assert ep.C_EP == 16.0 * max(ep.R_MEASURED, 1.0)


# ------------------------------------------------------------------ 3. one pass is MMSE
@pytest.mark.parametrize("si,vi", ep.CASES)
def test_one_pass_is_the_mmse_restatement(si, vi):
    c = ep.case(si, vi)
    a = ep.ref(si, vi, 1)
    m = lo.linear_ref(c["y"], c["psi"], c["cons"], c["theta"], ep.VARNS[vi] ** 2, c["n_tx"],
                      kind="mmse", labels=c["labels"], x_d_true=c["x"])
    rat = lo.ratios(a, m, c["cons"])
    print(f"{ep.SHAPES[si]} varn {ep.VARNS[vi]}: " + " ".join(f"{k} {v:.3g}" for k, v in rat.items()))
    assert set(rat) == {"x_soft", "nu", "post", "llr", "llr_maxlog", "moments"}
    assert max(rat.values()) <= lo.C
    assert np.array_equal(a["idx"], m["idx"]) and np.array_equal(a["err"], m["err"])
    assert not a["kept"].any() and not a["clamped"].any()      # one pass updates nothing


# ------------------------------------------------------------------ 4. EP helps detection
def test_ep_makes_fewer_symbol_errors_than_mmse():
    """i.i.d. Rayleigh 8 x 8, 16-QAM, sigma2 = the noise the data carry, one channel draw per
    channel use (192 channels, 1536 symbols per case): no more errors than MMSE at 16 dB or 22 dB,
    at most 70 % of MMSE's in total (483 -> 251 and 220 -> 12 on these seeds, chosen on the CPU;
    the other seeds tried gave 491 -> 285, 514 -> 308 and 170 -> 18, 199 -> 18)."""
    tot_m = tot_e = 0
    for snr, seed in ep.DETECT_CASES:
        c = ep.detect_case(snr, seed)
        args = (c["y"], c["psi"], c["cons"], c["theta"], c["sigma2"], c["n_tx"])
        m = ep.symbol_errors(lo.linear_ref(*args, kind="mmse"), c)
        e = ep.symbol_errors(ep.ep_ref(*args), c)
        print(f"{snr} dB: MMSE {m}, EP {e} symbol errors of {c['x'].size}")
        assert e <= m
        tot_m, tot_e = tot_m + m, tot_e + e
    assert tot_e <= 0.7 * tot_m


# ------------------------------------------------------------------ 5. EP helps the chain
@pytest.mark.parametrize("shape", [eo.S56, eo.S88, eo.S68], ids=eo.chain_id)
def test_ep_chain_beats_the_soft_mmse_chain(shape):
    """varn = 0.3, 4 iterations: per trial no worse than 1.02 x the MMSE_SOFT chain's NMSE, and at
    most 0.7 x on the mean (0.65, 0.17 and 0.32 on these batches)."""
    c = eo.batch(shape, 0)
    mm = np.array(ep.mmse_chain_nmse(shape))
    en = np.array([eo.nmse_of(c, b, r["thetas"][-1]) for b, r in enumerate(ep.chain_ref(shape))])
    print(f"{shape}: EP " + " ".join(f"{v:.3e}" for v in en) + "; MMSE_SOFT "
          + " ".join(f"{v:.3e}" for v in mm) + f"; mean ratio {en.mean() / mm.mean():.3f}")
    assert np.all(en <= 1.02 * mm)
    assert en.mean() <= 0.7 * mm.mean()


# ------------------------------------------------------------------ 6. chain conditioning
@pytest.mark.parametrize("shape", ep.CHAIN_SHAPES, ids=eo.chain_id)
def test_chain_is_well_conditioned(shape):
    """Over every iteration of the seeded chain and of its perturbed copy: no failed pivot, no
    update within 1e-6 of r' = 0, and a relative 1e-13 perturbation of theta0 grows by at most
    1e3.  The bar the GPU tier holds theta to, 64 eps kappa max(growth, 1), stays below 1e-7."""
    for b, r in enumerate(ep.chain_ref(shape)):
        print(f"{shape} trial {b}: max cond(A) {r['kappa']:.3g}, margin_r {r['margin_r']:.3g}, "
              f"perturbation x {r['growth']:.3g}, bar {r['bar']:.3g}")
        assert not r["fail"]
        assert r["margin_r"] >= 1e-6
        assert r["growth"] <= 1e3
        assert r["bar"] <= 1e-7


# ------------------------------------------------------------------ 7. the header
def test_header_defines():
    src = open(HEADER).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert val("SBCE_ESTEP_EP") == 10 and val("SBCE_LINEAR_EP") == 3
    assert val("SBCE_ABI_VERSION") == 7
    assert "#define SBCE_LINEAR_EP_PASSES(n) (((n) & 0xff) << 8)" in src
    assert not re.search(r"#define SBCE_ESTEP_\w+ 9\b", src)
    assert not re.search(r"#define SBCE_LINEAR_\w+ 2\b", src)


def test_python_constants_match_the_header(sbce):
    L = sbce._lib
    assert (L.SBCE_ESTEP_EP, L.SBCE_LINEAR_EP) == (10, 3)
    assert L.linear_ep_passes(5) == 5 << 8 and L.linear_ep_passes(0) == 0
    em = __import__(sbce.__name__ + ".em", fromlist=["em"])
    assert em._MODES["ep"] == 10 and em._LINEAR_KINDS["ep"] == 3
    assert em._mode_word("ep", 3, None) == 0 and em._mode_word("ep", 3, 7) == 7
    assert em._mode_word("pm", 3, None) == 3 and em._mode_word("ep", 0, 16) == 16
    for bad in (-1, 17, 256, 257):
        with pytest.raises(ValueError):
            em._mode_word("ep", 0, bad)
    with pytest.raises(ValueError):
        em._mode_word("mmse_soft", 0, 5)
    assert "ep" in sbce.sweeps.SNR_DETECTORS and callable(sbce.em_ep)
