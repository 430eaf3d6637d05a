"""CPU tier of linear soft detection (sbce_detect_linear): the conditions the GPU parity test
relies on, the bounds' constant measured against a 50-digit copy of the restatement, identities
that tie the restatement to the exhaustive detector's, the ABI and every validation return code
without a GPU, and the sweep's host logic with the restatement in place of the device call.

The constant of the bounds (tests/linear_oracle.py, `scales`): r = 17.65, the largest ratio of
|float64 restatement - 50-digit restatement| to eps kappa_t scale over every parity case and
output (x_soft of the MMSE case (8,4,5,9,4) at varn 0.3; all other cases and outputs < 4), so
C = 16 max(r, 1) = 282.4."""
import ctypes
import inspect
import os
import re
import subprocess
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT
import detect_oracle as dorc
import linear_oracle as lo

HEADER = os.path.join(ROOT, "include", "sbce.h")


# ------------------------------------------------------------------ 1. the parity cases
@pytest.mark.parametrize("si,vi,kind", lo.CASES)
def test_parity_cases_are_well_conditioned(si, vi, kind):
    o = lo.ref(si, vi, kind)
    assert not o["fail"].any() and not o["status"].any()
    assert o["kappa"].max() <= 1e4, o["kappa"].max()
    assert o["gap"].min() >= 1e-6, o["gap"].min()
    assert np.all(np.isfinite(o["nu"])) and np.all(o["nu"] > 0)
    assert np.allclose(o["post"].sum(axis=-1), 1.0, atol=1e-12)
    assert np.array_equal(o["x_hat"], lo.case(si, vi)["cons"][o["idx"]])


def test_parity_shapes_are_the_listed_ones():
    assert lo.SHAPES == [(1, 1, 1, 3, 4), (2, 2, 3, 5, 16), (3, 8, 33, 18, 4), (5, 6, 3, 17, 16),
                         (7, 8, 9, 20, 64), (8, 8, 5, 24, 16), (8, 4, 5, 9, 4), (4, 8, 5, 16, 2)]
    assert lo.VARNS == [0.3, 1.0] and lo.B == 3
    assert [k for s, v, k in lo.CASES if s == 6] == ["mmse", "mmse"]        # n_rx < n_tx
    assert len(lo.CASES) == 2 * (7 * 2 + 1)
    cons, lab = lo.table(2)
    assert list(lab) == [1, 0] and abs(cons[0] + cons[1]) > 0.1           # no grid, no identity


@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_multi_workgroup_case_meets_the_same_conditions(kind):
    """T_d = 70 spans three 32-symbol workgroups; trial 1's ZF matrix is singular from symbol 40
    on, and nowhere else is any pivot lost."""
    o = lo.chunk_ref(kind)
    want = np.zeros((3, 70), bool)
    if kind == "zf":
        want[1, lo.DEFECT_T0:] = True
    assert np.array_equal(o["fail"], want)
    assert list(o["status"]) == ([0, lo.NONHPD, 0] if kind == "zf" else [0, 0, 0])
    ok = ~o["fail"]
    assert o["kappa"][ok].max() <= 1e4 and o["gap"][ok].min() >= 1e-6
    assert lo.CHUNK_SHAPE[3] > 64 and lo.CHUNK_SHAPE[3] % 32 and 32 <= lo.DEFECT_T0


def test_zero_channel_column_of_the_restatement():
    """MMSE with a zero column: mu = 0 for that stream alone; no NaN, no status bit."""
    c = lo.case(1, 0)                                      # (2,2,3,5,16)
    th = c["theta"].copy().reshape(3, 3, 2, 2)
    th[0, :, 1, :] = 0.0
    r = lo.linear_ref(c["y"], c["psi"], c["cons"], th.reshape(3, -1), 0.09, 2, kind="mmse",
                      labels=c["labels"])
    assert not r["status"].any() and not r["fail"].any()
    assert np.all(r["x_soft"][0, :, 1] == 0) and np.all(r["nu"][0, :, 1] >= 1e12)
    assert np.allclose(r["post"][0, :, 1], 1.0 / 16, rtol=0, atol=1e-12)
    assert np.abs(r["llr"][0, :, 1]).max() <= 1e-10
    for k in ("x_soft", "post", "llr", "moments"):
        assert np.all(np.isfinite(r[k])), k
    assert np.all(np.isfinite(r["nu"][0, :, 0])) and np.all(np.isfinite(r["nu"][1:]))


# ------------------------------------------------------------------ 2. the constant
def test_constant_against_extended_precision():
    """r over all parity cases and outputs; C = 16 max(r, 1) is what linear_oracle.C holds."""
    worst, where = 0.0, None
    for si, vi, kind in lo.CASES:
        c, o = lo.case(si, vi), lo.ref(si, vi, kind)
        m = lo.linear_ref_mp(c["y"], c["psi"], c["cons"], c["theta"], lo.VARNS[vi] ** 2, c["n_tx"],
                             kind, lo.default_es(c["cons"]), c["labels"])
        for k, v in lo.ratios(m, o, c["cons"]).items():
            if v > worst:
                worst, where = v, (lo.SHAPES[si], lo.VARNS[vi], kind, k)
    print(f"r = {worst:.3f} at {where}; C = {lo.C}")
    assert worst <= lo.R_MEASURED
    assert worst >= 0.9 * lo.R_MEASURED          # the recorded figure is the measured one
    assert lo.C == 16.0 * max(lo.R_MEASURED, 1.0)


# ------------------------------------------------------------------ 3. identities
def _close(a, b, D, s2):
    return np.all(np.abs(a - b) <= 1e-11 * (1.0 + np.asarray(D) / s2)[..., None, None])


@pytest.mark.parametrize("kind,es", [("mmse", None), ("mmse", 1.0), ("mmse", 0.07), ("zf", None)])
def test_one_stream_is_the_exhaustive_detector(kind, es):
    """n_tx = 1: ||y - h x||^2 = |h|^2 |x_soft - x|^2 + const and nu = sigma2 / |h|^2, whatever
    the MMSE prior: post and llr are those of the joint detector."""
    rs = np.random.RandomState(5)
    n_rx, P, T, M = 3, 2, 7, 16
    cons, lab = lo.table(M)
    theta = rs.randn(2, P * n_rx) + 1j * rs.randn(2, P * n_rx)
    psi = np.exp(2j * np.pi * rs.rand(2, T, P))
    y = rs.randn(2, T, n_rx) + 1j * rs.randn(2, T, n_rx)
    s2 = 0.37
    e = dorc.detect_ref(y, psi, cons, theta, s2, 1, labels=lab)
    r = lo.linear_ref(y, psi, cons, theta, s2, 1, kind=kind, es=es, labels=lab)
    assert np.array_equal(r["idx"], e["idx"])
    assert _close(r["post"], e["post"], e["D"], s2)
    assert _close(r["llr"], e["llr"], e["D"], s2)
    assert _close(r["llr_maxlog"], e["llr_maxlog"], e["D"], s2)


@pytest.mark.parametrize("kind", ["mmse", "zf"])
def test_orthogonal_columns_are_the_exhaustive_detector(kind):
    """H = a scaled unitary (n_tx = 3, M = 4, P = 1, psi = 1): the joint posterior factorises."""
    rs = np.random.RandomState(8)
    n, T, M = 3, 6, 4
    cons, lab = lo.table(M)
    q, _ = np.linalg.qr(rs.randn(n, n) + 1j * rs.randn(n, n))
    H = 1.7 * q                                            # H[r][a]
    theta = H.T.reshape(1, -1)                             # theta[(0 n + a) n + r]
    psi = np.ones((1, T, 1), complex)
    x = cons[rs.randint(0, M, size=(1, T, n))]
    y = np.einsum("ra,bta->btr", H, x) + 0.3 * (rs.randn(1, T, n) + 1j * rs.randn(1, T, n))
    s2 = 0.5
    e = dorc.detect_ref(y, psi, cons, theta, s2, n, labels=lab)
    r = lo.linear_ref(y, psi, cons, theta, s2, n, kind=kind, labels=lab)
    assert np.array_equal(r["idx"], e["idx"])
    assert _close(r["post"], e["post"], e["D"], s2)
    assert _close(r["llr"], e["llr"], e["D"], s2)


def test_failed_pivot_rule_of_the_restatement():
    c = lo.case(3, 0)
    th = c["theta"].copy().reshape(3, 3, 5, 6)
    th[1, :, 3, :] = th[1, :, 1, :]                        # trial 1: streams 1 and 3 coincide
    r = lo.linear_ref(c["y"], c["psi"], c["cons"], th.reshape(3, -1), 0.09, 5, kind="zf",
                      labels=c["labels"])
    assert list(r["status"]) == [0, lo.NONHPD, 0] and r["fail"][1].all() and not r["fail"][0].any()
    assert np.all(r["x_soft"][1] == 0) and np.all(np.isinf(r["nu"][1]))
    assert np.all(r["post"][1] == 1.0 / 16) and np.all(r["llr"][1] == 0)
    assert np.all(r["idx"][1] == np.argmin(np.abs(c["cons"]) ** 2))


# ------------------------------------------------------------------ ABI
def _fields(cname):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*;", body)


def test_header_exports_and_ctypes_agree(sbce):
    L = sbce._lib
    src = open(HEADER).read()
    assert int(re.search(r"#define SBCE_ABI_VERSION (\d+)", src).group(1)) == 7
    for name in ("sbce_detect_linear_workspace_bytes", "sbce_detect_linear"):
        assert name in L.EXPORTED
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert _fields("sbce_linear_dims") == [f for f, _ in L.LinearDims._fields_]
    assert _fields("sbce_linear_ptrs") == [f for f, _ in L.LinearPtrs._fields_]
    assert "#define SBCE_LINEAR_MMSE 0" in src and L.SBCE_LINEAR_MMSE == 0
    assert "#define SBCE_LINEAR_ZF 1" in src and L.SBCE_LINEAR_ZF == 1


def test_struct_layout_matches_c(sbce, tmp_path):
    L = sbce._lib
    dn = [f for f, _ in L.LinearDims._fields_]
    pn = [f for f, _ in L.LinearPtrs._fields_]
    items = (["sizeof(sbce_linear_dims)", "sizeof(sbce_linear_ptrs)"]
             + [f"offsetof(sbce_linear_dims, {f})" for f in dn]
             + [f"offsetof(sbce_linear_ptrs, {f})" for f in pn])
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sbce.h"\n'
                     "int main(void) {\n"
                     + "".join(f'  printf("%zu\\n", (size_t){it});\n' for it in items)
                     + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out == ([ctypes.sizeof(L.LinearDims), ctypes.sizeof(L.LinearPtrs)]
                   + [getattr(L.LinearDims, f).offset for f in dn]
                   + [getattr(L.LinearPtrs, f).offset for f in pn])


def _dims(L, **over):
    v = dict(batch=2, n_tx=5, n_rx=6, n_psi=5, t_d=12, m=16, kind=L.SBCE_LINEAR_MMSE, flags=0,
             sigma2=0.01, es=10.0)
    v.update(over)
    return L.LinearDims(*[v[f] for f, _ in L.LinearDims._fields_])


def _call(L, lib, dims=None, **ptr_over):
    vals = dict(y_d=256, psi_d=256, cons=256, theta=256, labels=None, sigma2_t=None, x_d_true=None,
                x_soft=256, nu=256, x_hat=256, idx_hat=256, post=256, llr=None, err=None,
                moments=256, status=256, workspace=None, workspace_bytes=0)
    vals.update(ptr_over)
    p = L.LinearPtrs(*[vals[f] for f, _ in L.LinearPtrs._fields_])
    return lib.sbce_detect_linear(ctypes.byref(dims or _dims(L)), ctypes.byref(p), None)


@pytest.mark.parametrize("ab", [False, True])
def test_validation_return_codes_without_gpu(sbce, ab):
    """Everything below is refused before any HIP call (this runs without a GPU)."""
    L = sbce._lib
    lib = L.load_ab() if ab else L.load()
    n = ctypes.c_size_t(7)
    assert lib.sbce_detect_linear_workspace_bytes(ctypes.byref(_dims(L)), ctypes.byref(n)) == 0
    assert n.value == 0
    assert lib.sbce_detect_linear_workspace_bytes(None, ctypes.byref(n)) == -1
    assert lib.sbce_detect_linear_workspace_bytes(ctypes.byref(_dims(L)), None) == -1
    assert lib.sbce_detect_linear(None, None, None) == -1
    for k in ("y_d", "psi_d", "cons", "theta"):
        assert _call(L, lib, **{k: None}) == -1, k
    for over in (dict(batch=0), dict(n_tx=0), dict(n_rx=0), dict(n_psi=0), dict(t_d=0), dict(m=1),
                 dict(m=6), dict(m=128), dict(sigma2=0.0), dict(sigma2=-1.0),
                 dict(sigma2=float("nan")), dict(es=0.0), dict(es=-2.0), dict(es=float("nan")),
                 dict(kind=2), dict(kind=-1), dict(flags=2), dict(flags=-1),
                 dict(kind=L.SBCE_LINEAR_ZF, n_tx=5, n_rx=4)):
        assert _call(L, lib, dims=_dims(L, **over)) == -1, over
    assert _call(L, lib, llr=256) == -1
    assert _call(L, lib, err=256, x_d_true=256) == -1
    assert _call(L, lib, err=256, labels=256) == -1
    for k, v in (("y_d", 264), ("psi_d", 264), ("cons", 8), ("theta", 264), ("x_hat", 264),
                 ("x_soft", 264), ("moments", 264), ("x_d_true", 264), ("post", 260), ("nu", 260),
                 ("sigma2_t", 260), ("idx_hat", 258), ("labels", 258), ("status", 258)):
        assert _call(L, lib, **{k: v}) == -1, k
    assert _call(L, lib, llr=260, labels=256) == -1
    assert _call(L, lib, err=258, labels=256, x_d_true=256) == -1
    # outside the compiled kernel set
    assert _call(L, lib, dims=_dims(L, n_tx=9, n_rx=8)) == -2
    assert _call(L, lib, dims=_dims(L, n_rx=9)) == -2
    assert _call(L, lib, dims=_dims(L, kind=L.SBCE_LINEAR_ZF, n_tx=9, n_rx=9)) == -2
    # ZF ignores es; n_rx < n_tx is fine for MMSE (no launch here: nothing past validation runs
    # without a device, so only the refusals are exercised)


# ------------------------------------------------------------------ 4. sweep host logic
def test_sweep_routes_linear_detectors(sbce, monkeypatch):
    sw = sbce.sweeps
    calls = {"em": [], "lin": [], "ml": 0}

    def fake_em(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", partition_r=0, **kw):
        calls["em"].append((mode, partition_r))
        return {"theta": np.asarray(theta0) * 0.97}

    def lin(*a, **kw):
        calls["lin"].append(kw["kind"])
        assert kw["want"] == () and kw["x_d_true"] is not None and kw["labels"] is not None
        return lo.oracle_detect_linear_batch(*a, **kw)

    def ml(*a, **kw):
        calls["ml"] += 1
        return dorc.oracle_detect_batch(*a, **kw)

    monkeypatch.setattr(sw, "em_batch", fake_em)
    monkeypatch.setattr(sw, "detect_linear_batch", lin)
    monkeypatch.setattr(sw, "detect_batch", ml)
    kw = dict(SNR=(0, 25), T_d=10, T_p=24, N=3, n_rx=6, n_tx=5, itera=2, monte_iter=3, M=4, seed=2)
    ests = ("pilot", "pm", "pm_soft", "zf", "mmse", "genie")
    snr, ser, ber, nmse = sw.detection_vs_snr(estimators=ests, detector="mmse", **kw)
    assert calls["ml"] == 0 and calls["lin"] == ["mmse"] * len(ests)
    assert [m for m, _ in calls["em"]] == ["pm", "pm_soft", "zf", "mmse"]
    assert list(snr) == [0, 25] and set(ser) == set(ber) == set(nmse) == set(ests)
    for e in ests:
        assert ser[e].shape == ber[e].shape == nmse[e].shape == (2,)
        assert np.all((0 <= ser[e]) & (ser[e] <= 1)) and np.all((0 <= ber[e]) & (ber[e] <= 1))
    assert ser["genie"][-1] <= ser["pilot"][-1]
    assert np.all(nmse["genie"] == 0.0)
    # the counts are the restatement's
    points, varns = sw.gen_snr(kw["SNR"], 10, 24, 3, 6, 5, 3, 4, 10.0, 2, True, 1.0)
    cons, lab = sbce.qam.qam_constellation(4), sbce.qam.gray_labeling(4)
    trials, vn = points[1], varns[1]
    y = np.stack([t["Y_d"] for t in trials])
    psi = np.stack([t["Psi_d"].T for t in trials])
    x = np.stack([t["X_d"] for t in trials])
    e = lo.linear_ref(y, psi, cons, np.stack([t["h"] for t in trials]), vn * vn, 5, kind="mmse",
                      labels=lab, x_d_true=x)["err"]
    assert ser["genie"][1] == e[:, 0].sum() / (3 * 10 * 5)
    assert ber["genie"][1] == e[:, 1].sum() / (3 * 10 * 5 * 2)
    # zf routes the same way
    calls["lin"].clear()
    sw.detection_vs_snr(estimators=("pilot", "genie"), detector="zf", **kw)
    assert calls["lin"] == ["zf", "zf"]
    # soft / hard enumerate M^n_tx hypotheses: beyond their limit they are refused
    for est in ("soft", "hard"):
        with pytest.raises(ValueError):
            sw.detection_vs_snr(estimators=("pilot", est), detector="mmse", **kw)
    with pytest.raises(ValueError):
        sw.detection_vs_snr(estimators=("pilot",), detector="sphere", **kw)
    # within the limit they run with a linear detector too
    kw2 = dict(kw, n_tx=2, n_rx=2)
    _, ser2, _, _ = sw.detection_vs_snr(estimators=("soft", "genie"), detector="mmse", **kw2)
    assert set(ser2) == {"soft", "genie"}
    # the default detector is the joint one
    sw.detection_vs_snr(estimators=("pilot",), **kw2)
    assert calls["ml"] == 1


# ------------------------------------------------------------------ 5. detect_batch unchanged
def test_detect_batch_default_path_is_unchanged(sbce, monkeypatch):
    import torch
    em = import_module(sbce.__name__ + ".em")
    seen = []

    def rec(*a):
        seen.append(a)
        return {"idx": "out"}

    def never(*a, **k):
        raise AssertionError("the linear call must not be reached")

    monkeypatch.setattr(em, "_torch", lambda: torch)
    monkeypatch.setattr(em, "_cdev", lambda t, x: x)
    monkeypatch.setattr(em, "_detect_call", rec)
    monkeypatch.setattr(em, "_detect_linear_call", never)
    y, psi = np.zeros((2, 3, 2), complex), np.ones((2, 3, 4), complex)
    cons, theta = np.exp(2j * np.pi * np.arange(8) / 8), np.ones((2, 16), complex)
    r = sbce.detect_batch(y, psi, cons, theta, 0.5, 2, want=("idx",), return_device=True)
    assert r == {"idx": "out"} and len(seen) == 1
    a = seen[0]
    assert a[0] is torch and a[1] is y and a[2] is psi and a[3] is cons and a[4] is theta
    assert a[5:] == (2, 0.25, None, None, None, False, ("idx",))
    assert list(inspect.signature(sbce.detect_batch).parameters) == [
        "y_d", "psi_d", "cons", "theta", "varn", "n_tx", "labels", "x_d_true", "noise", "maxlog",
        "want", "return_device"]
    assert list(inspect.signature(sbce.detect).parameters) == [
        "Y_d", "PsiTilde_td", "all_possibleSymbols", "M", "varn", "theta", "labels", "X_d", "noise",
        "maxlog", "want"]
    assert list(inspect.signature(sbce.EMEngine.detect).parameters) == [
        "self", "labels", "x_d_true", "noise", "maxlog", "want", "return_device"]
    assert list(inspect.signature(sbce.detect_linear_batch).parameters) == [
        "y_d", "psi_d", "cons", "theta", "varn", "n_tx", "kind", "es", "labels", "x_d_true",
        "noise", "maxlog", "want", "return_device"]


def test_python_layer_argument_checks_without_gpu(sbce):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(sbce.SbceUnavailable):
            sbce.detect_linear_batch(np.zeros((1, 2, 1), complex), np.ones((1, 2, 1), complex),
                                     np.array([1, -1], complex), np.ones((1, 1), complex), 0.1, 1,
                                     want=("idx",))
