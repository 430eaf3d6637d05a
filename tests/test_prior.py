"""CPU tier of soft-input expectation propagation (sbce_detect_linear_prior, sbce_estep_prior,
sbce_em_prior): what the NumPy restatement (tests/prior_oracle.py) must satisfy whatever the
kernels do -- it is the prior-free restatement at zero L-values, exact at one stream, extrinsic at
one pass, and at the matched-filter bound under known interferers -- the guards the GPU parity
tests (tests/test_gpu_prior.py) rely on, the bounds' constants measured against a 50-digit copy,
the helpers of qam.py and the ABI's declarations."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from detect_oracle import bits_of
import ep_oracle as ep
import linear_em_oracle as eo
import linear_oracle as lo
import prior_oracle as po
from oracle.em_reduced import mstep_build

HEADER = os.path.join(ROOT, "include", "sbce.h")
CSRC = os.path.join(ROOT, po.PKG, "csrc")


def _held(got, o, cons, keys):
    """Each named output of `got` within its C_k eps kappa scale of the restatement result o."""
    rat = po.ratios({k: got[k] for k in keys}, o, cons)
    for k, v in rat.items():
        assert v <= po.C_BY_OUTPUT[k], (k, v)
    return rat


# ------------------------------------------------------------------ 1. zero L-values
@pytest.mark.parametrize("si,vi", [(1, 0), (3, 1), (5, 0), (6, 0)])
def test_zero_prior_reproduces_the_prior_free_restatement(si, vi):
    """On the zero-mean QAM tables the prior's moments are (0, es): the start, every weight and so
    every output are those of ep_oracle.ep_ref."""
    c, o = ep.case(si, vi), ep.ref(si, vi)
    la = np.zeros(c["x"].shape + (bits_of(c["labels"]).shape[1],))
    r = po.ep_prior_ref(c["y"], c["psi"], c["cons"], c["theta"], ep.VARNS[vi] ** 2, c["n_tx"], la,
                        labels=c["labels"], x_d_true=c["x"])
    rat = lo.ratios(r, o, c["cons"])
    print(f"{ep.SHAPES[si]} varn {ep.VARNS[vi]}: " + " ".join(f"{k} {v:.3g}" for k, v in rat.items()))
    assert max(rat.values()) <= 1.0
    assert np.array_equal(r["idx"], o["idx"]) and np.array_equal(r["err"], o["err"])


# ------------------------------------------------------------------ 2. one stream is exact
@pytest.mark.parametrize("passes", [1, 3, 5])
def test_one_stream_posterior_is_bayes(passes):
    """n_tx = 1: post is the exact posterior ~ pi(s) e^{-||y - h c_s||^2 / s2} for any p; random
    L-values, one of them +inf."""
    rs = np.random.RandomState(3)
    cons, labels = lo.table(16)
    n_rx, T, s2 = 4, 12, 0.5
    h = (rs.randn(n_rx) + 1j * rs.randn(n_rx)) / np.sqrt(2)
    x = cons[rs.randint(0, 16, T)]
    y = h[None, :] * x[:, None] + np.sqrt(s2 / 2) * (rs.randn(T, n_rx) + 1j * rs.randn(T, n_rx))
    la = 3.0 * rs.randn(1, T, 1, 4)
    la[0, 2, 0, 1] = np.inf
    theta = h[None, :]                                      # P = 1, n_tx = 1: theta[r] = h[r]
    o = po.ep_prior_ref(y[None], np.ones((1, T, 1), complex), cons, theta, s2, 1, la,
                        passes=passes, labels=labels)
    lp = np.stack([po.prior_lp(po.sanitise(la[0, t]), bits_of(labels))[0] for t in range(T)])
    zz = -np.sum(np.abs(y[:, None, :] - h[None, None, :] * cons[None, :, None]) ** 2, axis=2) / s2 + lp
    bayes = np.exp(zz - zz.max(axis=1, keepdims=True))
    bayes /= bayes.sum(axis=1, keepdims=True)
    rat = _held(dict(post=bayes[None, :, None, :]), o, cons, ("post",))
    print(f"p {passes}: post vs Bayes / (eps kappa scale) {rat['post']:.3g}, max kappa "
          f"{o['kappa'].max():.3g}")
    assert not o["fail"].any() and not o["dead"].any()


# ------------------------------------------------------------------ 3. extrinsic at one pass
def test_own_prior_independence_at_one_pass():
    """p = 1: x_soft_a and nu_a do not depend on La[a][.], llr[a][i] not on La[a][i]."""
    si, vi, ii = 3, 0, 0
    c, o = po.case(si, vi, ii), po.ref(si, vi, ii, 1)
    a, i = 2, 1
    la = np.array(c["la"])
    la2 = la.copy()
    la2[:, :, a, :] = np.random.RandomState(5).randn(*la2[:, :, a, :].shape) * 4.0
    la3 = la.copy()
    la3[:, :, a, i] = -la3[:, :, a, i] + 1.5
    run = lambda v: po.ep_prior_ref(c["y"], c["psi"], c["cons"], c["theta"], po.VARNS[vi] ** 2,
                                    c["n_tx"], v, passes=1, labels=c["labels"])
    r2, r3 = run(la2), run(la3)
    sc = po.scales(o, c["cons"])
    e_x = np.abs(r2["x_soft"][:, :, a] - o["x_soft"][:, :, a])
    e_n = np.abs(r2["nu"][:, :, a] - o["nu"][:, :, a])
    fin = np.isfinite(np.array(c["la"])[:, :, a, i])        # a planted +-inf or NaN is re-mapped
    e_l = np.abs(r3["llr"][:, :, a, i] - o["llr"][:, :, a, i])[fin]
    print(f"own-prior change: x_soft {e_x.max():.2e}, nu {e_n.max():.2e}, llr {e_l.max():.2e}")
    assert np.all(e_x <= po.C_BY_OUTPUT["x_soft"] * sc["x_soft"][:, :, a])
    assert np.all(e_n <= po.C_BY_OUTPUT["nu"] * sc["nu"][:, :, a])
    assert np.all(e_l <= (po.C_BY_OUTPUT["llr"] * sc["llr"][:, :, a, 0])[fin])
    assert np.abs(r2["x_soft"] - o["x_soft"]).max() > 1e-6     # the other streams do move


# ------------------------------------------------------------------ 4. known interferers
def test_known_interferers_reach_the_matched_filter_bound():
    """Streams c != a known (prior_llr_known), stream a without prior.  p = 1:
    s2 / ||h_a||^2 <= nu_a <= 1 / (||h_a||^2 / s2 - delta), delta = kEpVarFloor es
    sum_c |h_a^H h_c|^2 / s2^2 (the interference the variance floor leaves); p = 5: the relative
    excess over the matched-filter bound is at most twice the p = 1 excess."""
    si, vi, a = 3, 0, 1                                     # (5,6,3,17,16), varn 0.3
    c = lo.case(si, vi)
    n_tx, n_rx, P, T_d, M = lo.SHAPES[si]
    s2, es = lo.VARNS[vi] ** 2, lo.default_es(c["cons"])
    la = po.qam.prior_llr_known(c["x"], c["cons"], c["labels"])
    la[:, :, a, :] = 0.0
    H = np.einsum("btp,bpar->btra", c["psi"], c["theta"].reshape(lo.B, P, n_tx, n_rx))
    ha2 = np.sum(np.abs(H[:, :, :, a]) ** 2, axis=2)
    cross = np.abs(np.einsum("btr,btrc->btc", H[:, :, :, a].conj(), H)) ** 2
    cross[:, :, a] = 0.0
    delta = po.VFLOOR * es * cross.sum(axis=2) / s2 ** 2
    mf, up = s2 / ha2, 1.0 / (ha2 / s2 - delta)
    run = lambda p: po.ep_prior_ref(c["y"], c["psi"], c["cons"], c["theta"], s2, n_tx, la, passes=p,
                                    labels=c["labels"])["nu"][:, :, a]
    nu1, nu5 = run(1), run(5)
    ex1, ex5, exb = (nu1 / mf - 1).max(), (nu5 / mf - 1).max(), (up / mf - 1).max()
    print(f"relative excess over the matched-filter bound: p = 1 {ex1:.4e} (bound {exb:.4e}), "
          f"p = 5 {ex5:.4e}")
    tol = 1e-12
    assert np.all(nu1 >= mf * (1 - tol)) and np.all(nu1 <= up * (1 + tol))
    assert np.all(nu5 >= mf * (1 - tol)) and ex5 <= 2.0 * ex1


# ------------------------------------------------------------------ 5. guards of the parity cases
@pytest.mark.parametrize("passes", po.PASSES)
@pytest.mark.parametrize("si,vi,ii", po.CASES)
def test_parity_cases_cannot_flip_a_branch(si, vi, ii, passes):
    """No failed pivot, no dead stream; the channel's own conditioning cond(G + (s2 / es) I) <= 1e4
    (linear_oracle's seeds; the cond(A) of the passes themselves exceeds it by construction, a
    known bit or a decided stream having r_a = s2 / (5e-7 es), and enters the bound through
    kappa); test_ep.py's update margins; at most 1 % of the symbols with a relative MAP-decision
    gap below 1e-6; the four planted entries are where the case says."""
    c, o = po.case(si, vi, ii), po.ref(si, vi, ii, passes)
    small = (o["gap"] < po.GAP).any(axis=2)
    print(f"{po.SHAPES[si]} varn {po.VARNS[vi]} I_A {po.IAS[ii]} p {passes}: cond channel "
          f"{o['kappa0'].max():.3g}, passes {o['kappa'].max():.3g}, margin_r "
          f"{o['margin_r'].min():.3g}, margin_v {o['margin_v'].min():.3g}, gap {o['gap'].min():.3g}, "
          f"kept {o['kept'].sum()}, clamped {o['clamped'].sum()}")
    assert not o["fail"].any() and not o["status"].any() and not o["dead"].any()
    assert o["kappa0"].max() <= 1e4
    assert o["margin_r"].min() >= 1e-6 and o["margin_v"].min() >= 1e-3
    assert small.mean() <= 0.01
    assert np.all(np.isfinite(o["nu"])) and np.all(o["nu"] > 0)
    assert np.all(np.isfinite(o["llr"])) and np.all(np.isfinite(o["llr_maxlog"]))
    assert np.allclose(o["post"].sum(axis=-1), 1.0, atol=1e-12)
    flat = np.asarray(c["la"]).reshape(-1)
    n = flat.size
    assert flat[0] == np.inf and flat[n // 3] == -np.inf and np.isnan(flat[n // 2])
    assert flat[n - 1] == 1e3 and np.abs(o["la"]).max() == po.CLAMP
    assert len({0, n // 3, n // 2, n - 1}) == 4


def test_multi_workgroup_case_fails_where_planted():
    """T_d = 70 with |La| <= 4: exactly trial 1's symbols from DEFECT_T0 on lose a pivot (a
    numerical rank deficiency of the inputs); they carry the a-priori pmf, llr = 0, x_soft = 0 and
    nu = inf; the other symbols hold the guards."""
    o = po.chunk_ref()
    want = np.zeros((3, 70), bool)
    want[1, lo.DEFECT_T0:] = True
    assert np.array_equal(o["fail"], want) and list(o["status"]) == [0, lo.NONHPD, 0]
    assert np.abs(po.chunk_la()).max() <= 4.0
    assert np.array_equal(o["post"][want], o["prior"][want])
    assert np.all(o["llr"][want] == 0) and np.all(o["x_soft"][want] == 0)
    assert np.all(o["nu"][want] == np.inf)
    ok = ~want
    assert o["margin_r"][ok].min() >= 1e-6 and o["margin_v"][ok].min() >= 1e-3
    assert o["gap"][ok].min() >= po.GAP and not o["dead"][ok].any()


# ------------------------------------------------------------------ 6. the constants
def test_constants_against_extended_precision():
    """r_k over every parity case and both pass counts; C_k = 16 max(r_k, 1) is what prior_oracle
    holds."""
    by, where = {}, {}
    for si, vi, ii in po.CASES:
        for p in po.PASSES:
            c, o = po.case(si, vi, ii), po.ref(si, vi, ii, p)
            m = po.ep_prior_ref_mp(c["y"], c["psi"], c["cons"], c["theta"], po.VARNS[vi] ** 2,
                                   c["n_tx"], c["la"], p, lo.default_es(c["cons"]), c["labels"])
            for k, v in po.ratios(m, o, c["cons"]).items():
                if v > by.get(k, 0.0):
                    by[k], where[k] = v, (po.SHAPES[si], po.VARNS[vi], po.IAS[ii], p)
    print("r_k: " + ", ".join(f"{k} {v:.5g} at {where[k]}" for k, v in by.items()))
    assert set(by) == set(po.R_BY_OUTPUT)
    for k, v in by.items():
        assert 0.9 * po.R_BY_OUTPUT[k] <= v <= po.R_BY_OUTPUT[k], (k, v)
        assert po.C_BY_OUTPUT[k] == 16.0 * max(po.R_BY_OUTPUT[k], 1.0)


# ------------------------------------------------------------------ 7. the chain
@pytest.mark.parametrize("shape", po.CHAIN_SHAPES, ids=eo.chain_id)
def test_chain_is_well_conditioned(shape):
    for b, r in enumerate(po.chain_ref(shape)):
        print(f"{shape} trial {b}: max cond(A) {r['kappa']:.3g}, margin_r {r['margin_r']:.3g}, "
              f"perturbation x {r['growth']:.3g}, bar {r['bar']:.3g}")
        assert not r["fail"]
        assert r["margin_r"] >= 1e-6
        assert r["growth"] <= 1e3
        assert r["bar"] <= 1e-7


@pytest.mark.parametrize("shape", [eo.S56, eo.S88], ids=eo.chain_id)
def test_known_symbols_reach_the_genie_bound(shape):
    """I_A = 1 (prior_llr_known): one restated iteration is the genie M-step, so its NMSE averaged
    over the batch lies within 4 standard deviations of the genie Cramer-Rao bound n_rx s2
    tr(R^-1) / ||h||^2; theta_hat - theta ~ CN(0, s2 R^-1) per receive row gives ||.||^2 the
    variance n_rx s2^2 tr(R^-2).  The spread printed here is what the GPU tier computes too."""
    c = eo.batch(shape, 0)
    lab = po.chain_labels(c)
    la = po.qam.prior_llr_known(c["x_d"], c["cons"], lab)
    s2, n_rx = c["varn"] ** 2, c["n_rx"]
    nm, bound, var = [], [], []
    for b in range(eo.B):
        th = po.chain(c, b, 1, la)["thetas"][-1]
        x = c["x_d"][b]
        R, _ = mstep_build(c["u_p"][b], c["y_p"][b], c["psi_d"][b].T, c["y_d"][b], x,
                           x[:, :, None] * x[:, None, :].conj())
        Ri = np.linalg.inv(R)
        hn = np.linalg.norm(c["h"][b]) ** 2
        nm.append(eo.nmse_of(c, b, th))
        bound.append(n_rx * s2 * np.real(np.trace(Ri)) / hn)
        var.append(n_rx * s2 * s2 * np.real(np.trace(Ri @ Ri)) / hn ** 2)
    spread = np.sqrt(np.sum(var)) / eo.B
    print(f"{shape}: mean NMSE {np.mean(nm):.4e}, genie bound {np.mean(bound):.4e}, spread of the "
          f"mean {spread:.2e}")
    assert abs(np.mean(nm) - np.mean(bound)) <= 4.0 * spread


# ------------------------------------------------------------------ 8. helpers
def test_prior_helpers(sbce):
    q = sbce.qam
    cons, labels = lo.table(16)
    rs = np.random.RandomState(0)
    idx = rs.randint(0, 16, (3, 5, 2))
    la = q.prior_llr_known(cons[idx], cons, labels)
    assert la.shape == (3, 5, 2, 4) and np.all(np.isinf(la))
    assert np.array_equal(la < 0, bits_of(labels)[idx] == 1)
    lp = po.prior_lp(po.sanitise(la[0, 0]), bits_of(labels))
    assert np.array_equal(np.argmax(lp, axis=1), idx[0, 0])
    bits = rs.randint(0, 2, 200000)
    assert not q.prior_llr_gaussian(bits, 0.0, rs).any()
    one = q.prior_llr_gaussian(bits, 1.0, rs)
    assert np.array_equal(one, np.where(bits == 0, np.inf, -np.inf))
    assert q.bit_mutual_information(one, bits) == 1.0
    assert q.bit_mutual_information(np.zeros(bits.shape), bits) == 0.0
    for ia in (0.1, 0.5, 0.9):
        sig = q._j_inverse(ia)
        assert abs((1 - 2 ** (-0.3073 * sig ** 1.787)) ** 1.1064 - ia) <= 1e-12
        got = q.bit_mutual_information(q.prior_llr_gaussian(bits, ia, rs), bits)
        print(f"I_A {ia}: sigma {sig:.4f}, measured {got:.4f}")
        assert abs(got - ia) <= 0.01          # the J approximation's error plus 2e5 samples
    with pytest.raises(ValueError):
        q.prior_llr_gaussian(bits, 1.5, rs)


# ------------------------------------------------------------------ 9. the declarations
def test_header_and_binding(sbce):
    src = open(HEADER).read()
    assert int(re.search(r"#define SBCE_ABI_VERSION (\d+)", src).group(1)) == 7
    body = re.search(r"typedef struct sbce_prior_opts \{(.*?)\} sbce_prior_opts;", src, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    L = sbce._lib
    assert fields == [f for f, _ in L.PriorOpts._fields_] == ["la", "labels", "flags"]
    for name in ("sbce_detect_linear_prior", "sbce_estep_prior", "sbce_em_prior"):
        assert name in L.EXPORTED and hasattr(L.load(), name)
    dev = open(os.path.join(CSRC, "ep_prior.h")).read()
    assert float(re.search(r"kPriorClamp = ([\d.]+)", dev).group(1)) == po.CLAMP
    internal = open(os.path.join(CSRC, "sbce_internal.h")).read()
    args = re.search(r"struct EstepArgs \{(.*?)\n\};", internal, re.S).group(1)
    members = re.findall(r"(\w+)(?: = [\w.]+)?;", re.sub(r"//.*", "", args))
    assert members[-2:] == ["la", "labels"]               # trailing, default null
    # no prior: nothing of the prior is touched without a GPU either
    import ctypes
    d = L.Dims(1, 2, 2, 3, 4, 8, 4, 0, 0.1)
    assert L.load().sbce_em_prior(ctypes.byref(d), ctypes.byref(L.Ptrs()), 1, L.SBCE_ESTEP_EP, 0,
                                  None, None, None, None) == -1
