"""GPU tier of the Gaussian-approximation comparator EM (csrc/approx.hip, sbce_approx_em):
parity with the reference's own EM_approx ("Comparision/Comparision T_d vs NMSE.py":106-145)
on every fixture case, one update against the NumPy restatement, batch independence, per-trial
variances, the drop-in, the singular normal matrix, and the two comparison sweeps against the
reference-run fixture curves."""
import numpy as np
import pytest

import approx_oracle as ao
from conftest import golden, rel

pytestmark = pytest.mark.gpu

NAMES = ("Psi_p", "Psi_d", "x_p", "Y_p", "Y_d", "G0")
SWEEP_TAGS = [("comparison_td", "td20"), ("comparison_td", "td100"),
              ("comparison_tp", "tp4"), ("comparison_tp", "tp40")]


def _small(k, prefix="c"):
    d = golden("approx_small")
    c = {name: d[f"{prefix}{k}_{name}"] for name in NAMES}
    if prefix == "c":
        c["G_hat"] = d[f"c{k}_G_hat"]
        c["iters"], c["varn"] = int(d["shapes"][k][4]), float(d["shapes"][k][5])
    return c


def _run(sbce, c, updates, varn):
    b = ao.batch_major(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], c["G0"])
    return sbce.em_approx_batch(b["y_d"], b["y_p"], b["psi_d"], b["psi_p"], b["x_p"], varn,
                                updates, b["g0"])


@pytest.mark.parametrize("k", range(6))
def test_fixture_parity_small(sbce, k):
    """Odd shapes (N below, at, just over 32 and at 64; M = 1; T_d no multiple of the chunk;
    T_p < N and > N; varn = 1.0, where a Hermitian-only solve is off by 1e-1): G within 1e-9 of
    the reference's, status 0."""
    c = _small(k)
    r = _run(sbce, c, c["iters"] + 1, c["varn"])
    e = rel(r["g"][0], c["G_hat"])
    print(f"case {k}: rel {e:.2e}")
    assert r["status"][0] == 0
    assert e < 1e-9, (k, e)


@pytest.mark.parametrize("name,tag", SWEEP_TAGS)
def test_fixture_parity_sweep_points(sbce, name, tag):
    d = golden(name)
    c = dict(Psi_p=d[f"{tag}_Psi_p"], Psi_d=d[f"{tag}_Psi_d"], x_p=d[f"{tag}_x_p"],
             Y_p=d[f"{tag}_Y_p_dft"], Y_d=d[f"{tag}_Y_d_dft"], G0=d[f"{tag}_G0"])
    r = _run(sbce, c, int(d["itera"]) + 1, float(d["varn"]))
    e = rel(r["g"][0], d[f"{tag}_G_hat"])
    print(f"{tag}: rel {e:.2e}")
    assert r["status"][0] == 0
    assert e < 1e-9, (tag, e)


@pytest.mark.parametrize("k", [0, 2])
def test_one_update_matches_restatement(sbce, k):
    """updates = 1 on (6,2,4,9) and (33,5,7,65) against the restatement's first update: 1e-11
    (the project holds normal equations to 1e-12..1e-13; cond(A) <= 341 here)."""
    c = _small(k)
    G1 = ao.em_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], 1, c["varn"], G0=c["G0"])
    r = _run(sbce, c, 1, c["varn"])
    e = rel(r["g"][0], G1)
    print(f"case {k}: one update rel {e:.2e}")
    assert r["status"][0] == 0 and e < 1e-11, (k, e)


def _three(sbce):
    cs = [_small(s, prefix="s") for s in range(3)]
    bs = [ao.batch_major(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], c["G0"]) for c in cs]
    return {key: np.concatenate([b[key] for b in bs]) for key in bs[0]}


def test_batch_independence_bitwise(sbce):
    """300 trials (three different (6,2,4,9) trials, tiled): every output equals, bitwise, the
    B = 1 result of the same trial."""
    b3 = _three(sbce)
    single = [sbce.em_approx_batch(*(b3[k][i:i + 1] for k in ("y_d", "y_p", "psi_d", "psi_p", "x_p")),
                                   0.1, 4, b3["g0"][i:i + 1])["g"][0] for i in range(3)]
    big = {k: np.tile(v, (100,) + (1,) * (v.ndim - 1)) for k, v in b3.items()}
    r = sbce.em_approx_batch(big["y_d"], big["y_p"], big["psi_d"], big["psi_p"], big["x_p"], 0.1, 4,
                             big["g0"])
    assert r["g"].shape[0] == 300 and not r["status"].any()
    for i in range(300):
        assert np.array_equal(r["g"][i].view(np.float64), single[i % 3].view(np.float64)), i
    assert not np.array_equal(single[0], single[1])


def test_per_trial_variances_bitwise(sbce):
    """Two variances in one call give, bitwise, the results of two separate calls."""
    b3 = _three(sbce)
    two = {k: v[:2] for k, v in b3.items()}
    args = lambda b: (b["y_d"], b["y_p"], b["psi_d"], b["psi_p"], b["x_p"])  # noqa: E731
    r = sbce.em_approx_batch(*args(two), np.array([0.1, 0.3]), 4, two["g0"])
    for i, v in enumerate((0.1, 0.3)):
        one = {k: x[i:i + 1] for k, x in two.items()}
        s = sbce.em_approx_batch(*args(one), v, 4, one["g0"])
        assert np.array_equal(r["g"][i].view(np.float64), s["g"][0].view(np.float64)), i
    same = sbce.em_approx_batch(*args(two), 0.1, 4, two["g0"])
    assert not np.array_equal(same["g"][1], r["g"][1])


def test_drop_in_runs_iterations_plus_one_updates(sbce):
    """EM_approx with the reference's argument layouts returns the fixture's G at 1e-9; the
    Iterations = 3 fixture tells 3 updates from 4."""
    c = _small(0)
    assert c["iters"] == 3
    G = sbce.EM_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], c["iters"], c["varn"],
                       np.zeros_like(c["G0"]))
    assert G.shape == c["G0"].shape and G.dtype == np.complex128
    assert rel(G, c["G_hat"]) < 1e-9
    G3 = ao.em_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], 3, c["varn"])
    assert rel(G3, c["G_hat"]) > 1e-6 and rel(G, G3) > 1e-6


def test_singular_normal_matrix_is_flagged(sbce):
    """(N, M, T_p, T_d) = (8,3,2,3): T_p + T_d < N, A is singular.  Every trial is flagged
    SBCE_STATUS_SINGULAR, G stays finite, the call returns 0; no parity is claimed."""
    rng = np.random.default_rng(5)
    B, N, M, Tp, Td = 5, 8, 3, 2, 3
    cx = lambda *s: (rng.normal(size=s) + 1j * rng.normal(size=s)) / np.sqrt(2)  # noqa: E731
    psi_d, psi_p = np.exp(2j * np.pi * rng.random((B, Td, N))), np.exp(2j * np.pi * rng.random((B, Tp, N)))
    x_p = np.exp(0.5j * np.pi * rng.integers(0, 4, (B, Tp)))
    g0 = cx(B, N, M)
    r = sbce.em_approx_batch(cx(B, Td, M), cx(B, Tp, M), psi_d, psi_p, x_p, 0.1, 4, g0)
    assert np.all(r["status"] & sbce._lib.SBCE_STATUS_SINGULAR)
    assert np.all(np.isfinite(r["g"].view(np.float64)))
    assert np.array_equal(r["g"], g0)       # singular at the first update: G_0 is the last iterate


def test_comparison_sweeps_reproduce_reference_curves(sbce):
    """comparison_vs_td / comparison_vs_tp at the fixtures' points (the scripts' constants, seed
    0, one trial) reproduce both curves: each NMSE within 1e-9 relative."""
    d = golden("comparison_td")
    x, cv = sbce.sweeps.comparison_vs_td(T_d=(20, 100), monte_iter=1, seed=0)
    for i, td in enumerate((20, 100)):
        for leg in ("proposed", "approx"):
            ref = float(d[f"td{td}_nmse_{leg}"])
            print(f"T_d {td} {leg}: {cv[leg][i]:.12e} ref {ref:.12e}")
            assert abs(cv[leg][i] / ref - 1) < 1e-9, (td, leg)
    d = golden("comparison_tp")
    x, cv = sbce.sweeps.comparison_vs_tp(T_p=(4, 40), monte_iter=1, seed=0)
    for i, tp in enumerate((4, 40)):
        for leg in ("proposed", "approx"):
            ref = float(d[f"tp{tp}_nmse_{leg}"])
            print(f"T_p {tp} {leg}: {cv[leg][i]:.12e} ref {ref:.12e}")
            assert abs(cv[leg][i] / ref - 1) < 1e-9, (tp, leg)
