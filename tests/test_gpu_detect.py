"""GPU tier of the batched detector / soft demapper (csrc/detect.hip, sbce_detect): parity with
the NumPy restatement on every shape, the reference modem's own L-values, agreement with the
existing E-step kernels on the same theta, log-domain safety, batch independence, per-trial
sigma^2, the counters and optional outputs, graph capture and the sweep.

Bounds: decisions exact; post 1e-11 (the project's E-step bar); L-values 1e-11 (1 + D / sigma^2)
with D the symbol's largest hypothesis distance (distance rounding ~50 eps D, divided by
sigma^2)."""
import functools
import itertools
from importlib import import_module

import numpy as np
import pytest

import detect_oracle as orc
from conftest import golden

pytestmark = pytest.mark.gpu

G = golden("detect")
SHAPES = [tuple(int(v) for v in s) for s in G["shapes"]]
VARNS = [float(v) for v in G["varns"]]
CASES = [(si, vi) for si in range(len(SHAPES)) for vi in range(len(VARNS))]


def case(si, vi=0):
    n_tx, n_rx, P, T_d, M = SHAPES[si]
    key = f"s{si}_labels"
    lab = G[key] if key in G.files else orc.gray_labeling(M)
    return dict(y=G[f"s{si}_y{vi}"], psi=G[f"s{si}_psi"], cons=G[f"s{si}_cons"],
                theta=G[f"s{si}_theta"], x=G[f"s{si}_x"], labels=lab, n_tx=n_tx, M=M)


@functools.lru_cache(maxsize=None)
def ref(si, vi, sigma2):
    """The restatement's result of a case, computed once and shared (never modified)."""
    c = case(si, vi)
    r = orc.detect_ref(c["y"], c["psi"], c["cons"], c["theta"], sigma2, c["n_tx"],
                       labels=c["labels"], x_d_true=c["x"])
    for v in r.values():
        v.setflags(write=False)
    return r


def run(sbce, c, varn, **kw):
    kw.setdefault("labels", c["labels"])
    return sbce.detect_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], **kw)


def llr_bound(D, sigma2):
    return 1e-11 * (1.0 + np.asarray(D) / sigma2)[..., None, None]


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("si,vi", CASES)
def test_parity_with_restatement(sbce, si, vi):
    c, varn = case(si, vi), VARNS[vi]
    s2 = varn * varn
    o = ref(si, vi, s2)
    r = run(sbce, c, varn, x_d_true=c["x"])
    rm = run(sbce, c, varn, maxlog=True, want=("llr",))
    e_post = np.abs(r["post"] - o["post"]).max()
    e_llr = np.abs(r["llr"] - o["llr"]) / llr_bound(o["D"], s2)
    e_ml = np.abs(rm["llr"] - o["llr_maxlog"]) / llr_bound(o["D"], s2)
    print(f"shape {SHAPES[si]} varn {varn}: post err {e_post:.2e}, llr err/bound {e_llr.max():.2e} "
          f"(abs {np.abs(r['llr'] - o['llr']).max():.2e}), maxlog err/bound {e_ml.max():.2e}, "
          f"max D/s2 {(o['D'] / s2).max():.2e}, max |llr| {np.abs(o['llr']).max():.2e}")
    assert np.array_equal(r["idx"], o["idx"])
    assert np.array_equal(r["x_hat"], o["x_hat"])
    assert r["idx"].dtype == np.int32
    assert e_post <= 1e-11
    assert np.all(e_llr <= 1.0)
    assert np.all(e_ml <= 1.0)
    assert np.array_equal(r["err"], o["err"])


# ------------------------------------------------------------------ 2. the reference's L-values
@pytest.mark.parametrize("M", [4, 16, 64])
def test_reference_modem_lvalues(sbce, M):
    """n_tx = n_rx = P = 1, theta = 1, sigma^2 = N0: llr is QAM.py's demodulate(received, 'soft')."""
    rx = G[f"rx_{M}"]
    T = rx.size
    cons, lab = G[f"cons_{M}"], G[f"labeling_{M}"]
    for i, n0 in enumerate(G["n0s"]):
        n0 = float(n0)
        r = sbce.detect_batch(rx.reshape(1, T, 1), np.ones((1, T, 1), complex), cons,
                              np.ones((1, 1), complex), n0, 1, labels=lab, noise="true")
        D = (np.abs(rx[:, None] - cons[None, :]) ** 2).max(axis=1)
        err = np.abs(r["llr"][0, :, 0, :] - G[f"lvalues_{M}_{i}"]) / (1e-11 * (1 + D / n0))[:, None]
        print(f"M {M} N0 {n0}: llr err/bound {err.max():.2e}")
        assert np.all(err <= 1.0)
        # default labelling of a square-QAM-sized table = the modem's
        r2 = sbce.detect_batch(rx.reshape(1, T, 1), np.ones((1, T, 1), complex), cons,
                               np.ones((1, 1), complex), n0, 1, noise="true", want=("llr",))
        assert np.array_equal(r2["llr"], r["llr"])


# ------------------------------------------------------------------ 3. the existing kernels
@pytest.mark.parametrize("si,vi", CASES)
def test_agrees_with_estep_kernels(sbce, si, vi):
    c, varn = case(si, vi), VARNS[vi]
    r = run(sbce, c, varn, want=("x_hat", "post"))
    m_soft, _ = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], "soft")
    m_hard, _ = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"], "hard")
    mean = (r["post"] * c["cons"]).sum(axis=-1)
    e_soft = np.abs(mean - m_soft).max()
    e_hard = np.abs(r["x_hat"] - m_hard).max()
    print(f"shape {SHAPES[si]} varn {varn}: soft mean err {e_soft:.2e}, hard err {e_hard:.2e}")
    assert e_soft <= 1e-11 * np.abs(c["cons"]).max() ** 2
    assert e_hard <= 1e-12


# ------------------------------------------------------------------ 4. log-domain safety
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_log_domain_safety(sbce, si):
    """varn = 0.01 (sigma^2 = 1e-4, |LLR| ~ 1e6..1e7): a naive exp(-d / sigma^2) is 0 / 0."""
    c = case(si, 0)
    r = run(sbce, c, 0.01)
    rm = run(sbce, c, 0.01, maxlog=True, want=("llr",))
    base = run(sbce, c, 0.1, want=("idx", "x_hat"))
    print(f"shape {SHAPES[si]}: max |llr| {np.abs(r['llr']).max():.3e}, "
          f"post sum err {np.abs(r['post'].sum(axis=-1) - 1).max():.2e}")
    for k in ("x_hat", "post", "llr"):
        assert np.all(np.isfinite(r[k])), k
    assert np.all(np.isfinite(rm["llr"]))
    assert np.all(r["post"] >= 0)
    assert np.abs(r["post"].sum(axis=-1) - 1).max() <= 1e-12
    assert np.array_equal(r["idx"], base["idx"]) and np.array_equal(r["x_hat"], base["x_hat"])
    assert np.abs(r["llr"]).max() > 1e4


# ------------------------------------------------------------------ 5. batch independence
@pytest.mark.parametrize("si", [2, 3])
def test_batch_independence(sbce, si):
    """300 trials (the three trials tiled) are bitwise the B = 1 results; T_d = 9 and 7 leave
    ragged tails in the symbol chunks."""
    c = case(si, 0)
    big = {k: np.tile(c[k], (100,) + (1,) * (c[k].ndim - 1)) for k in ("y", "psi", "theta", "x")}
    rb = sbce.detect_batch(big["y"], big["psi"], c["cons"], big["theta"], 0.1, c["n_tx"],
                           labels=c["labels"], x_d_true=big["x"])
    for b in range(3):
        one = sbce.detect_batch(c["y"][b:b + 1], c["psi"][b:b + 1], c["cons"], c["theta"][b:b + 1],
                                0.1, c["n_tx"], labels=c["labels"], x_d_true=c["x"][b:b + 1])
        for k in ("idx", "x_hat", "post", "llr", "err"):
            got = rb[k][b::3]
            assert np.array_equal(got, np.broadcast_to(one[k], got.shape)), (k, b)


# ------------------------------------------------------------------ 6. per-trial sigma^2
@pytest.mark.parametrize("noise", ["em", "true"])
def test_per_trial_sigma2(sbce, noise):
    c = case(1, 0)
    vt = np.array([0.1, 1.0, 0.3])
    r = run(sbce, c, vt, noise=noise, x_d_true=c["x"])
    for b in range(3):
        one = sbce.detect_batch(c["y"][b:b + 1], c["psi"][b:b + 1], c["cons"], c["theta"][b:b + 1],
                                float(vt[b]), c["n_tx"], labels=c["labels"], noise=noise,
                                x_d_true=c["x"][b:b + 1])
        for k in ("idx", "x_hat", "post", "llr", "err"):
            assert np.array_equal(r[k][b:b + 1], one[k]), (k, b)


# ------------------------------------------------------------------ 7. counters, optional outputs
@pytest.mark.parametrize("si", [1, 7, 8])
def test_counters_and_optional_outputs(sbce, si):
    c = case(si, 1)                                   # varn = 1.0: decisions do go wrong
    full = run(sbce, c, 1.0, x_d_true=c["x"])
    assert np.array_equal(full["err"], orc.count_errors(full["idx"], c["cons"], c["x"], c["labels"]))
    assert full["err"].dtype == np.int32 and full["err"].shape == (3, 2)
    # against "true" symbols that are each one table step off the decisions, every entry counts
    off = c["cons"][(full["idx"] + 1) % c["M"]]
    wrong = run(sbce, c, 1.0, x_d_true=off, want=("idx",))
    assert np.all(wrong["err"][:, 0] == full["idx"][0].size)
    assert np.array_equal(wrong["err"], orc.count_errors(full["idx"], c["cons"], off, c["labels"]))
    assert "err" not in run(sbce, c, 1.0)             # no x_d_true: no counter
    names = ("x_hat", "idx", "llr", "post")
    for n in range(len(names) + 1):
        for want in itertools.combinations(names, n):
            r = run(sbce, c, 1.0, want=want, x_d_true=c["x"])
            assert set(r) == set(want) | {"err"}
            for k in r:
                assert np.array_equal(r[k], full[k]), (want, k)


def test_tables_without_default_labelling(sbce):
    c = case(8, 0)                                    # 8-PSK
    with pytest.raises(ValueError):
        run(sbce, c, 0.1, labels=None)
    with pytest.raises(ValueError):
        run(sbce, c, 0.1, labels=None, want=("idx",), x_d_true=c["x"])
    r = run(sbce, c, 0.1, labels=None, want=("idx", "post"))
    assert np.array_equal(r["idx"], ref(8, 0, VARNS[0] * VARNS[0])["idx"])


def test_single_trial_front_end_and_engine(sbce):
    c = case(1, 0)
    aps = sbce.qam.all_possible_symbols(c["cons"], c["n_tx"])
    full = run(sbce, c, 0.1, x_d_true=c["x"])
    Y_d = [y[:, None] for y in c["y"][0]]
    r = sbce.detect(Y_d, c["psi"][0].T, aps, c["M"], 0.1, c["theta"][0].reshape(-1, 1),
                    X_d=[x[:, None] for x in c["x"][0]])
    for k in ("idx", "x_hat", "post", "llr", "err"):
        assert np.array_equal(r[k], full[k][0]), k
    n_rx, P = c["y"].shape[2], c["psi"].shape[2]
    batch = dict(y_d=c["y"], y_p=np.zeros((3, 1, n_rx), complex), psi_d=c["psi"],
                 u_p=np.zeros((3, 1, P * c["n_tx"]), complex), cons=c["cons"], theta0=c["theta"])
    eng = sbce.EMEngine(batch, 0.1, x_d_true=c["x"])
    e = eng.detect()
    for k in ("idx", "x_hat", "post", "llr", "err"):
        assert np.array_equal(e[k], full[k]), k


# ------------------------------------------------------------------ 8. graph capture
def test_graph_capture_replays_the_eager_bits(sbce):
    import torch
    em = import_module(sbce.__name__ + ".em")
    c = case(4, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(c["x"])).cuda()
    args = (torch, *dev, c["n_tx"], 0.01, None, lab, xd, False, ("x_hat", "idx", "llr", "post"))
    eager = {k: v.cpu().numpy() for k, v in em._detect_call(*args).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = em._detect_call(*args)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert np.array_equal(out[k].cpu().numpy(), v), k


# ------------------------------------------------------------------ 9. the sweep
def test_sweep_matches_restatement_driven_sweep(sbce, monkeypatch):
    sw = sbce.sweeps
    kw = dict(SNR=(5, 15), T_d=12, T_p=6, N=4, n_rx=2, n_tx=2, itera=3, monte_iter=4, M=4,
              estimators=("pilot", "soft", "hard", "genie"), seed=5)
    snr, ser, ber, nmse = sw.detection_vs_snr(**kw)
    monkeypatch.setattr(sw, "detect_batch", orc.oracle_detect_batch)
    snr2, ser2, ber2, nmse2 = sw.detection_vs_snr(**kw)
    n_sym = 4 * 12 * 2
    for e in kw["estimators"]:
        print(e, "ser", ser[e], "ber", ber[e], "nmse", nmse[e])
        assert np.array_equal(np.rint(ser[e] * n_sym), np.rint(ser2[e] * n_sym))
        assert np.array_equal(ser[e], ser2[e]) and np.array_equal(ber[e], ber2[e])
        assert np.allclose(nmse[e], nmse2[e], rtol=1e-9, atol=0)
    assert np.all(nmse["genie"] == 0)
    assert np.all(ser["genie"] <= ser["pilot"])
