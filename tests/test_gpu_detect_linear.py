"""GPU tier of linear soft detection (csrc/detect_linear.hip, sbce_detect_linear): parity with the
NumPy restatement on every shape, kind and noise level, agreement with the shipped exhaustive
detector and E-step where the two coincide, log-domain safety, batch independence, per-trial
sigma^2, the failed-pivot rule, optional outputs, error codes and graph capture.

Bounds (tests/linear_oracle.py): decisions and counters exact (the CPU tier asserts a relative
gap >= 1e-6 between each stream's two nearest table points); continuous outputs within
C eps kappa_t scale with C = 16 max(r, 1) = 282.4, r = 17.65 measured on the CPU against a
50-digit copy of the restatement (tests/test_detect_linear.py); nothing comes from the kernel."""
import itertools
from importlib import import_module

import numpy as np
import pytest

import detect_oracle as dorc
import linear_oracle as lo

pytestmark = pytest.mark.gpu

ALL = ("x_soft", "nu", "x_hat", "idx", "llr", "post", "moments", "status")
KEYS = ALL + ("err",)


def run(sbce, c, varn, kind, **kw):
    kw.setdefault("labels", c["labels"])
    kw.setdefault("want", ALL)
    return sbce.detect_linear_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"],
                                    kind=kind, **kw)


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("si,vi,kind", lo.CASES)
def test_parity_with_restatement(sbce, si, vi, kind):
    c, varn, o = lo.case(si, vi), lo.VARNS[vi], lo.ref(si, vi, kind)
    r = run(sbce, c, varn, kind, x_d_true=c["x"])
    rm = run(sbce, c, varn, kind, maxlog=True, want=("llr",))
    got = dict(r, llr_maxlog=rm["llr"])
    rat = lo.ratios(got, o, c["cons"])
    print(f"shape {lo.SHAPES[si]} varn {varn} {kind}: max kappa {o['kappa'].max():.3g}, "
          "err / (eps kappa scale): " + ", ".join(f"{k} {v:.3g}" for k, v in rat.items())
          + f" (bound {lo.C})")
    assert np.array_equal(r["idx"], o["idx"]) and r["idx"].dtype == np.int32
    assert np.array_equal(r["x_hat"], o["x_hat"])
    assert np.array_equal(r["err"], o["err"])
    assert np.array_equal(r["status"], o["status"])
    assert set(rat) == {"x_soft", "nu", "post", "llr", "llr_maxlog", "moments"}
    for k, v in rat.items():
        assert v <= lo.C, (k, v)


# ------------------------------------------------------------------ 2. the shipped detector
def _joint_cases():
    rs = np.random.RandomState(21)
    cons, lab = lo.table(16)
    n_rx, P, T = 4, 3, 9
    theta = (rs.randn(3, P * n_rx) + 1j * rs.randn(3, P * n_rx)) / np.sqrt(2 * P)
    psi = np.exp(2j * np.pi * rs.rand(3, T, P))
    H = np.einsum("btp,bpr->btr", psi, theta.reshape(3, P, n_rx))
    x = cons[rs.randint(0, 16, size=(3, T, 1))]
    y = H * x + 0.3 * (rs.randn(3, T, n_rx) + 1j * rs.randn(3, T, n_rx)) / np.sqrt(2)
    one = dict(y=y, psi=psi, cons=cons, labels=lab, theta=theta, n_tx=1)
    cons, lab = lo.table(4)
    n, T = 4, 10                                           # J = 4^4 = 256
    theta = np.zeros((3, n * n), complex)
    for b in range(3):
        q, _ = np.linalg.qr(rs.randn(n, n) + 1j * rs.randn(n, n))
        theta[b] = ((1.0 + b) * q).T.reshape(-1)           # theta[(0 n + a) n + r] = H[r][a]
    psi = np.ones((3, T, 1), complex)
    Hm = theta.reshape(3, n, n).transpose(0, 2, 1)
    x = cons[rs.randint(0, 4, size=(3, T, n))]
    y = np.einsum("bra,bta->btr", Hm, x) + 0.3 * (rs.randn(3, T, n) + 1j * rs.randn(3, T, n))
    return {"one": one, "orth": dict(y=y, psi=psi, cons=cons, labels=lab, theta=theta, n_tx=n)}


@pytest.mark.parametrize("name", ["one", "orth"])
@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_agrees_with_exhaustive_detector(sbce, name, kind):
    """n_tx = 1, and orthogonal channel columns at n_tx = 4: the joint posterior factorises into
    the per-stream ones, so the shipped sbce_detect gives the same post and llr."""
    c, varn = _joint_cases()[name], 0.5
    o = lo.linear_ref(c["y"], c["psi"], c["cons"], c["theta"], varn * varn, c["n_tx"], kind=kind,
                      labels=c["labels"])
    r = run(sbce, c, varn, kind, want=("idx", "post", "llr"))
    e = sbce.detect_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, c["n_tx"],
                          labels=c["labels"], want=("idx", "post", "llr"))
    sc = lo.scales(o, c["cons"])
    rat = {k: float(np.max(np.abs(r[k] - e[k]) / sc[k])) for k in ("post", "llr")}
    print(f"{name} {kind}: vs sbce_detect err / (eps kappa scale): {rat} (bound {lo.C})")
    assert np.array_equal(r["idx"], e["idx"])
    assert rat["post"] <= lo.C and rat["llr"] <= lo.C


# ------------------------------------------------------------------ 3. the E-step and the M-step
@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_one_stream_moments_are_the_soft_estep(sbce, kind):
    c, varn = _joint_cases()["one"], 0.5
    r = run(sbce, c, varn, kind, want=("moments",))
    m, S = sbce.estep_batch(c["y"], c["psi"], c["cons"], c["theta"], varn, 1, "soft")
    bar = 1e-11 * np.abs(c["cons"]).max() ** 2
    e_m, e_S = np.abs(r["moments"][..., :1] - m).max(), np.abs(r["moments"][..., 1] - S[..., 0, 0]).max()
    print(f"{kind}: m err {e_m:.2e}, S err {e_S:.2e}, bar {bar:.2e}")
    assert e_m <= bar and e_S <= bar


def test_mstep_accepts_the_moments(sbce):
    si = 3                                                 # (5,6,3,17,16)
    c = lo.case(si, 0)
    n_tx, n_rx, P, T_d, M = lo.SHAPES[si]
    r = run(sbce, c, 0.3, "mmse", want=("moments",))
    m = r["moments"][..., :n_tx]
    S = r["moments"][..., n_tx:].reshape(3, T_d, n_tx, n_tx)
    assert np.allclose(S, np.conj(np.swapaxes(S, 2, 3)), rtol=0, atol=1e-12)
    rs = np.random.RandomState(3)
    T_p, L = 20, P * n_tx
    u_p = (rs.randn(3, T_p, L) + 1j * rs.randn(3, T_p, L)) / np.sqrt(2)
    Hc = c["theta"].reshape(3, L, n_rx)
    y_p = np.einsum("btl,blr->btr", u_p, Hc) + 0.3 * (rs.randn(3, T_p, n_rx) + 1j * rs.randn(3, T_p, n_rx))
    th, R, rhs, st = sbce.mstep_batch(c["y"], y_p, c["psi"], u_p, c["cons"], m, S, 0.3)
    rel = np.linalg.norm(th - c["theta"]) / np.linalg.norm(c["theta"])
    print(f"theta after one M-step from the linear moments: rel distance to the truth {rel:.3f}")
    assert th.shape == c["theta"].shape and np.all(np.isfinite(th))
    assert not (st & sbce._lib.SBCE_STATUS_NONHPD).any()


# ------------------------------------------------------------------ 4. log-domain safety
@pytest.mark.parametrize("si", range(len(lo.SHAPES)))
def test_log_domain_safety(sbce, si):
    """varn = 0.01 (sigma^2 = 1e-4, |LLR| up to ~1e6): a naive exp(-d / nu) is 0 / 0."""
    c = lo.case(si, 0)
    bits = dorc.bits_of(c["labels"])
    for kind in lo.kinds_of(lo.SHAPES[si]):
        r = run(sbce, c, 0.01, kind)
        rm = run(sbce, c, 0.01, kind, maxlog=True, want=("llr",))
        print(f"shape {lo.SHAPES[si]} {kind}: max |llr| {np.abs(r['llr']).max():.3e}, min |llr| "
              f"{np.abs(r['llr']).min():.3e}, post sum err {np.abs(r['post'].sum(axis=-1) - 1).max():.2e}")
        for k in ("x_soft", "nu", "x_hat", "post", "llr", "moments"):
            assert np.all(np.isfinite(r[k])), k
        assert np.all(np.isfinite(rm["llr"])) and not r["status"].any()
        assert np.all(r["post"] >= 0) and np.all(r["nu"] > 0)
        assert np.abs(r["post"].sum(axis=-1) - 1).max() <= 1e-12
        sign = np.where(bits[r["idx"]] == 0, 1.0, -1.0)     # bit 0 decided: L-value > 0
        assert np.array_equal(np.sign(r["llr"]), sign)
        assert np.array_equal(np.sign(rm["llr"]), sign)


# ------------------------------------------------------------------ 5. batch independence
@pytest.mark.parametrize("si,kind", [(2, "zf"), (3, "mmse"), (5, "mmse")])
def test_batch_independence(sbce, si, kind):
    c = lo.case(si, 0)
    full = run(sbce, c, 0.3, kind, x_d_true=c["x"])
    one = sbce.detect_linear_batch(c["y"][1:2], c["psi"][1:2], c["cons"], c["theta"][1:2], 0.3,
                                   c["n_tx"], kind=kind, labels=c["labels"], x_d_true=c["x"][1:2],
                                   want=ALL)
    for k in KEYS:
        assert np.array_equal(full[k][1:2], one[k]), k


# ------------------------------------------------------------------ 6. per-trial sigma^2
@pytest.mark.parametrize("kind,noise", [("mmse", "em"), ("zf", "true")])
def test_per_trial_sigma2(sbce, kind, noise):
    c = lo.case(3, 0)
    vt = np.array([0.1, 1.0, 0.3])
    r = run(sbce, c, vt, kind, noise=noise, x_d_true=c["x"])
    for b in range(3):
        one = sbce.detect_linear_batch(c["y"][b:b + 1], c["psi"][b:b + 1], c["cons"],
                                       c["theta"][b:b + 1], float(vt[b]), c["n_tx"], kind=kind,
                                       labels=c["labels"], noise=noise, x_d_true=c["x"][b:b + 1],
                                       want=ALL)
        for k in KEYS:
            assert np.array_equal(r[k][b:b + 1], one[k]), (k, b)


# ------------------------------------------------------------------ 7. rank-deficient ZF
def test_rank_deficient_zf(sbce):
    si = 3
    c = dict(lo.case(si, 0))
    n_tx, n_rx, P, T_d, M = lo.SHAPES[si]
    good = run(sbce, c, 0.3, "zf", x_d_true=c["x"])
    th = c["theta"].copy().reshape(3, P, n_tx, n_rx)
    th[1, :, 3, :] = th[1, :, 1, :]                        # trial 1: streams 1 and 3 coincide
    c["theta"] = th.reshape(3, -1)
    r = run(sbce, c, 0.3, "zf", x_d_true=c["x"])
    rm = run(sbce, c, 0.3, "zf", maxlog=True, want=("llr",))
    assert list(r["status"]) == [0, sbce._lib.SBCE_STATUS_NONHPD, 0]
    cons = c["cons"]
    i0 = int(np.argmin(np.abs(cons) ** 2))
    assert np.all(r["x_soft"][1] == 0) and np.all(r["nu"][1] == np.inf)
    assert np.all(r["post"][1] == 1.0 / M) and np.all(r["llr"][1] == 0) and np.all(rm["llr"][1] == 0)
    assert np.all(r["idx"][1] == i0) and np.all(r["x_hat"][1] == cons[i0])
    m = cons.sum() / M
    s = (np.abs(cons) ** 2).sum() / M
    mom = r["moments"][1]
    assert np.abs(mom[:, :n_tx] - m).max() <= 1e-15 * np.abs(cons).max()
    S = mom[:, n_tx:].reshape(T_d, n_tx, n_tx)
    off = ~np.eye(n_tx, dtype=bool)
    assert np.abs(S[:, ~off] - s).max() <= 4e-16 * s
    assert np.array_equal(S[:, off], np.broadcast_to((mom[:, :1] * np.conj(mom[:, :1])), (T_d, n_tx * n_tx - n_tx)))
    assert np.array_equal(r["err"][1], dorc.count_errors(r["idx"][1:2], cons, c["x"][1:2], c["labels"])[0])
    for b in (0, 2):
        for k in KEYS:
            assert np.array_equal(r[k][b], good[k][b]), (k, b)


# ------------------------------------------------------------------ 7b. several workgroups per trial
@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_several_workgroups_per_trial(sbce, kind):
    """T_d = 70: three 32-symbol workgroups per trial with a ragged last one.  Parity with the
    restatement in every chunk; err summed and status OR-ed over the workgroups of a trial (ZF:
    trial 1 is singular from symbol 40 on, so the flag comes from the second and third workgroup
    only); trial 1 of the batch is bitwise the B = 1 call."""
    c, o, varn = lo.chunk_case(), lo.chunk_ref(kind), lo.CHUNK_VARN
    n_tx, n_rx, P, T_d, M = lo.CHUNK_SHAPE
    r = run(sbce, c, varn, kind, x_d_true=c["x"])
    rm = run(sbce, c, varn, kind, maxlog=True, want=("llr",))
    ok = ~o["fail"]
    rat = lo.ratios(dict(r, llr_maxlog=rm["llr"]), o, c["cons"], ok=ok)
    print(f"T_d 70 {kind}: failed symbols {int(o['fail'].sum())}, err / (eps kappa scale): "
          + ", ".join(f"{k} {v:.3g}" for k, v in rat.items()) + f" (bound {lo.C})")
    assert np.array_equal(r["idx"], o["idx"]) and np.array_equal(r["x_hat"], o["x_hat"])
    assert np.array_equal(r["err"], o["err"]) and r["err"][:, 0].min() > 0
    assert np.array_equal(r["status"], o["status"])
    assert list(r["status"]) == ([0, sbce._lib.SBCE_STATUS_NONHPD, 0] if kind == "zf" else [0, 0, 0])
    assert set(rat) == {"x_soft", "nu", "post", "llr", "llr_maxlog", "moments"}
    for k, v in rat.items():
        assert v <= lo.C, (k, v)
    bad = o["fail"]                                        # the failed symbols, exactly
    assert bad.sum() == (T_d - lo.DEFECT_T0 if kind == "zf" else 0)
    assert np.all(r["x_soft"][bad] == 0) and np.all(r["nu"][bad] == np.inf)
    assert np.all(r["post"][bad] == 1.0 / M) and np.all(r["llr"][bad] == 0)
    assert np.all(rm["llr"][bad] == 0)
    assert np.abs(r["moments"][bad] - o["moments"][bad]).max(initial=0.0) <= 1e-14
    one = sbce.detect_linear_batch(c["y"][1:2], c["psi"][1:2], c["cons"], c["theta"][1:2], varn,
                                   n_tx, kind=kind, labels=c["labels"], x_d_true=c["x"][1:2],
                                   want=ALL)
    for k in KEYS:
        assert np.array_equal(r[k][1:2], one[k]), k


def test_zero_channel_column_mmse(sbce):
    """A zero channel column under MMSE: mu = 1 - rho g is 0 (or a few eps) for that stream alone.
    Its estimate is 0 with no information (nu = inf or of order 1 / eps), nothing is NaN, no
    status bit, and the other stream of the same symbols keeps the restatement's values."""
    c = dict(lo.case(1, 0))                                # (2,2,3,5,16)
    th = c["theta"].copy().reshape(3, 3, 2, 2)
    th[0, :, 1, :] = 0.0
    c["theta"] = th.reshape(3, -1)
    o = lo.linear_ref(c["y"], c["psi"], c["cons"], c["theta"], 0.09, 2, kind="mmse",
                      labels=c["labels"])
    r = run(sbce, c, 0.3, "mmse")
    assert not r["status"].any()
    assert np.all(r["x_soft"][0, :, 1] == 0) and np.all(r["nu"][0, :, 1] >= 1e12)
    assert np.abs(r["post"][0, :, 1] - 1.0 / 16).max() <= 1e-12
    assert np.abs(r["llr"][0, :, 1]).max() <= 1e-10
    for k in ("x_soft", "post", "llr", "moments"):
        assert np.all(np.isfinite(r[k])), k
    assert np.array_equal(r["idx"], o["idx"])
    keep = np.ones((3, 5, 2), bool)
    keep[0, :, 1] = False
    sc = lo.scales(o, c["cons"])
    assert np.all(np.isfinite(r["nu"][keep]))
    assert np.all(np.abs(r["x_soft"] - o["x_soft"])[keep] <= lo.C * sc["x_soft"][keep])
    assert np.all(np.abs(r["nu"][keep] - o["nu"][keep]) <= lo.C * sc["nu"][keep])
    assert np.all(np.abs(r["post"] - o["post"])[keep] <= lo.C * np.broadcast_to(sc["post"], r["post"].shape)[keep])


# ------------------------------------------------------------------ 8. optional outputs
def test_optional_outputs_and_counters(sbce):
    import torch
    c = lo.case(5, 1)                                      # varn = 1.0: decisions do go wrong
    full = run(sbce, c, 1.0, "mmse", x_d_true=c["x"])
    assert np.array_equal(full["err"], dorc.count_errors(full["idx"], c["cons"], c["x"], c["labels"]))
    assert full["err"].dtype == np.int32 and full["err"].shape == (3, 2) and full["err"][:, 0].min() > 0
    assert "err" not in run(sbce, c, 1.0, "mmse")
    subsets = [w for n in (0, 1, 7) for w in itertools.combinations(ALL, n)] + [("post", "nu"),
                                                                                 ("llr", "moments")]
    for want in subsets:
        r = run(sbce, c, 1.0, "mmse", want=want, x_d_true=c["x"])
        assert set(r) == set(want) | {"err"}
        for k in r:
            assert np.array_equal(r[k], full[k]), (want, k)
    # err and status are zeroed by the call: prefill through the raw binding
    L = sbce._lib
    lib = L.load()
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta", "x")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    err = torch.full((3, 2), 12345, dtype=torch.int32, device="cuda")
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    n_tx, n_rx, P, T_d, M = lo.SHAPES[5]
    dims = L.LinearDims(3, n_tx, n_rx, P, T_d, M, L.SBCE_LINEAR_MMSE, 0, 1.0, lo.default_es(c["cons"]))
    ptrs = L.LinearPtrs(y_d=dev[0].data_ptr(), psi_d=dev[1].data_ptr(), cons=dev[2].data_ptr(),
                        theta=dev[3].data_ptr(), labels=lab.data_ptr(), x_d_true=dev[4].data_ptr(),
                        err=err.data_ptr(), status=status.data_ptr())
    assert lib.sbce_detect_linear(dims, ptrs, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(err.cpu().numpy(), full["err"]) and not status.cpu().numpy().any()


def test_single_trial_front_end_and_engine(sbce):
    c = lo.case(3, 0)
    n_tx, n_rx, P, T_d, M = lo.SHAPES[3]
    full = run(sbce, c, 0.3, "zf", x_d_true=c["x"])
    Y_d = [y[:, None] for y in c["y"][0]]
    r = sbce.detect_linear(Y_d, c["psi"][0].T, c["cons"], M, 0.3, c["theta"][0].reshape(-1, 1),
                           kind="zf", labels=c["labels"], X_d=[x[:, None] for x in c["x"][0]])
    assert set(r) == {"x_soft", "nu", "x_hat", "idx", "llr", "post", "err"}
    for k in r:
        assert np.array_equal(r[k], full[k][0]), k
    batch =dict(y_d=c["y"], y_p=np.zeros((3, 1, n_rx), complex), psi_d=c["psi"],
                 u_p=np.zeros((3, 1, P * n_tx), complex), cons=c["cons"], theta0=c["theta"])
    eng = sbce.EMEngine(batch, 0.3, x_d_true=c["x"], mode="pm", partition_r=1)
    e = eng.detect_linear(kind="zf", labels=c["labels"])
    for k in e:
        assert np.array_equal(e[k], full[k]), k


# ------------------------------------------------------------------ 9. error codes
def test_error_codes_before_any_launch(sbce):
    import torch
    L = sbce._lib
    lib = L.load()
    c = lo.case(1, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    out = torch.full((3, 5, 2), -7.0, dtype=torch.float64, device="cuda")
    llr = torch.zeros((3, 5, 2, 4), dtype=torch.float64, device="cuda")

    def call(ptr_over=None, **over):
        v = dict(batch=3, n_tx=2, n_rx=2, n_psi=3, t_d=5, m=16, kind=L.SBCE_LINEAR_MMSE, flags=0,
                 sigma2=0.09, es=10.0)
        v.update(over)
        d = L.LinearDims(*[v[f] for f, _ in L.LinearDims._fields_])
        p = dict(y_d=dev[0].data_ptr(), psi_d=dev[1].data_ptr(), cons=dev[2].data_ptr(),
                 theta=dev[3].data_ptr(), nu=out.data_ptr())
        p.update(ptr_over or {})
        return lib.sbce_detect_linear(d, L.LinearPtrs(**p), torch.cuda.current_stream().cuda_stream)

    assert call(n_tx=9, n_rx=8) == -2
    assert call(n_rx=9) == -2
    assert call(kind=L.SBCE_LINEAR_ZF, n_tx=2, n_rx=1) == -1
    assert call(es=0.0) == -1 and call(es=-1.0) == -1
    assert call(sigma2=0.0) == -1 and call(sigma2=-0.5) == -1
    assert call(kind=2) == -1
    assert call({"y_d": dev[0].data_ptr() + 8}) == -1
    assert call({"nu": out.data_ptr() + 4}) == -1
    assert call({"llr": llr.data_ptr()}) == -1             # llr without labels
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)               # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() > 0)


# ------------------------------------------------------------------ 10. graph capture
def test_graph_capture_replays_the_eager_bits(sbce):
    import torch
    em = import_module(sbce.__name__ + ".em")
    c = lo.case(4, 0)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("y", "psi", "cons", "theta")]
    lab = torch.from_numpy(np.ascontiguousarray(c["labels"], dtype=np.int32)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(c["x"])).cuda()
    args = (torch, *dev, c["n_tx"], "mmse", 0.09, None, lo.default_es(c["cons"]), lab, xd, False, ALL)
    eager = {k: v.cpu().numpy() for k, v in em._detect_linear_call(*args).items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()                                # one stream: the graph is a linear chain
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = em._detect_linear_call(*args)
    for _ in range(2):
        for v in out.values():
            v.fill_(1)
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert np.array_equal(out[k].cpu().numpy(), v), k
