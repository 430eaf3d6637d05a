"""CPU tier of the batched detector / soft demapper (sbce_detect): the NumPy restatement against
the reference modem's recorded labelling and L-values, the ABI (header, exports, ctypes layouts),
every validation return code without a GPU, and the sweep's host logic with the restatement in
place of the device calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
import detect_oracle as orc

HEADER = os.path.join(ROOT, "include", "sbce.h")


def llr_bound(D, sigma2):
    """The project's 1e-11 bar scaled to an L-value: distance rounding ~50 eps D, divided by
    sigma^2."""
    return 1e-11 * (1.0 + np.asarray(D) / sigma2)


# ------------------------------------------------------------------ restatement vs reference
@pytest.mark.parametrize("M", [4, 16, 64])
def test_labelling_is_the_reference_modems(sbce, M):
    g = golden("detect")
    assert np.array_equal(orc.gray_labeling(M), g[f"labeling_{M}"])
    assert np.array_equal(sbce.qam.gray_labeling(M), g[f"labeling_{M}"])
    assert sbce.qam.gray_labeling(M).dtype == np.int32
    assert np.array_equal(sbce.qam.qam_constellation(M), g[f"cons_{M}"])
    bits = sbce.qam.bits_of(g[f"labeling_{M}"])
    assert bits.shape == (M, int(np.log2(M)))
    assert np.array_equal(bits, orc.bits_of(g[f"labeling_{M}"]))
    # LSB first: the label is recovered with weights 1, 2, 4, ...
    assert np.array_equal(bits.astype(np.int64) @ (1 << np.arange(bits.shape[1])),
                          g[f"labeling_{M}"])


def test_gray_labeling_rejects_non_square(sbce):
    with pytest.raises(ValueError):
        sbce.qam.gray_labeling(8)
    assert np.array_equal(sbce.qam.bits_of([0, 1]), [[0], [1]])


@pytest.mark.parametrize("M", [4, 16, 64])
def test_restatement_reproduces_reference_lvalues(M):
    """n_tx = n_rx = P = 1, theta = 1, sigma^2 = N0: the restatement's L-values are the modem's
    demodulate(received, 'soft') (QAM.py:164-185)."""
    g = golden("detect")
    rx = g[f"rx_{M}"]
    T = rx.size
    for i, n0 in enumerate(g["n0s"]):
        r = orc.detect_ref(rx.reshape(1, T, 1), np.ones((1, T, 1)), g[f"cons_{M}"],
                           np.ones((1, 1)), float(n0), 1, labels=g[f"labeling_{M}"])
        err = np.abs(r["llr"][0, :, 0, :] - g[f"lvalues_{M}_{i}"])
        assert np.all(err <= llr_bound(r["D"][0], float(n0))[:, None]), err.max()
        # and the hard decision is the modem's minimum-distance one
        assert np.array_equal(r["idx"][0, :, 0],
                              np.argmin(np.abs(rx[None, :] - g[f"cons_{M}"][:, None]), axis=0))


def test_restatement_is_consistent():
    g = golden("detect")
    si = 1
    cons, lab = g[f"s{si}_cons"], orc.gray_labeling(4)
    r = orc.detect_ref(g[f"s{si}_y0"], g[f"s{si}_psi"], cons, g[f"s{si}_theta"], 0.01, 2,
                       labels=lab, x_d_true=g[f"s{si}_x"])
    assert np.allclose(r["post"].sum(axis=-1), 1.0, atol=1e-12)
    assert np.array_equal(r["x_hat"], cons[r["idx"]])
    # max-log and exact L-values agree in sign and to log(J/2)
    assert np.all(np.abs(r["llr"] - r["llr_maxlog"]) <= np.log(8) + 1e-9)
    assert np.array_equal(r["err"], orc.count_errors(r["idx"], cons, g[f"s{si}_x"], lab))
    assert r["err"].shape == (3, 2)


# ------------------------------------------------------------------ ABI
def _fields(cname):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*;", body)


def test_header_exports_and_ctypes_agree(sbce):
    L = sbce._lib
    src = open(HEADER).read()
    ver = int(re.search(r"#define SBCE_ABI_VERSION (\d+)", src).group(1))
    assert ver == L.SBCE_ABI_VERSION
    for name in ("sbce_detect_workspace_bytes", "sbce_detect"):
        assert name in L.EXPORTED
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert _fields("sbce_detect_dims") == [f for f, _ in L.DetectDims._fields_]
    assert _fields("sbce_detect_ptrs") == [f for f, _ in L.DetectPtrs._fields_]
    assert "#define SBCE_DETECT_MAXLOG 1" in src and L.SBCE_DETECT_MAXLOG == 1


def test_detect_struct_layout_matches_c(sbce, tmp_path):
    """gcc's sizeof / offsetof of the two new structs against the ctypes binding."""
    L = sbce._lib
    dn = [f for f, _ in L.DetectDims._fields_]
    pn = [f for f, _ in L.DetectPtrs._fields_]
    items = (["sizeof(sbce_detect_dims)", "sizeof(sbce_detect_ptrs)"]
             + [f"offsetof(sbce_detect_dims, {f})" for f in dn]
             + [f"offsetof(sbce_detect_ptrs, {f})" for f in pn])
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
    expect = ([ctypes.sizeof(L.DetectDims), ctypes.sizeof(L.DetectPtrs)]
              + [getattr(L.DetectDims, f).offset for f in dn]
              + [getattr(L.DetectPtrs, f).offset for f in pn])
    assert out == expect


def _call(L, lib, dims=None, **ptr_over):
    d = dims or L.DetectDims(2, 2, 2, 5, 12, 4, 0, 0.01)
    vals = dict(y_d=256, psi_d=256, cons=256, theta=256, labels=None, sigma2_t=None, x_d_true=None,
                x_hat=256, idx_hat=256, post=256, llr=None, err=None, workspace=None,
                workspace_bytes=0)
    vals.update(ptr_over)
    p = L.DetectPtrs(*[vals[f] for f, _ in L.DetectPtrs._fields_])
    return lib.sbce_detect(ctypes.byref(d), ctypes.byref(p), None)


@pytest.mark.parametrize("ab", [False, True])
def test_validation_return_codes_without_gpu(sbce, ab):
    """Everything below is refused before any HIP call (this runs without a GPU); both library
    variants export the same entry points."""
    L = sbce._lib
    lib = L.load_ab() if ab else L.load()
    D = L.DetectDims
    n = ctypes.c_size_t(7)
    assert lib.sbce_detect_workspace_bytes(ctypes.byref(D(2, 2, 2, 5, 12, 4, 0, 0.01)),
                                           ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sbce_detect_workspace_bytes(None, ctypes.byref(n)) == -1
    assert lib.sbce_detect_workspace_bytes(ctypes.byref(D(2, 2, 2, 5, 12, 4, 0, 0.01)), None) == -1
    assert lib.sbce_detect(None, None, None) == -1
    # null required pointers
    for k in ("y_d", "psi_d", "cons", "theta"):
        assert _call(L, lib, **{k: None}) == -1, k
    # dims
    for bad in (D(0, 2, 2, 5, 12, 4, 0, 0.01), D(2, 2, 2, 5, 0, 4, 0, 0.01),
                D(2, 2, 2, 0, 12, 4, 0, 0.01), D(2, 0, 2, 5, 12, 4, 0, 0.01),
                D(2, 2, 0, 5, 12, 4, 0, 0.01),
                D(2, 2, 2, 5, 12, 1, 0, 0.01), D(2, 2, 2, 5, 12, 6, 0, 0.01),
                D(2, 2, 2, 5, 12, 128, 0, 0.01), D(2, 2, 2, 5, 12, 4, 0, 0.0),
                D(2, 2, 2, 5, 12, 4, 0, -1.0), D(2, 2, 2, 5, 12, 4, 0, float("nan")),
                D(2, 2, 2, 5, 12, 4, 2, 0.01), D(2, 2, 2, 5, 12, 4, -1, 0.01)):
        assert _call(L, lib, dims=bad) == -1, [getattr(bad, f) for f, _ in D._fields_]
    # llr / err need labels, err needs x_d_true
    assert _call(L, lib, llr=256) == -1
    assert _call(L, lib, err=256, x_d_true=256) == -1
    assert _call(L, lib, err=256, labels=256) == -1
    # misaligned pointers: 16 bytes complex, 8 float64, 4 int32
    for k, v in (("y_d", 264), ("psi_d", 264), ("cons", 8), ("theta", 264), ("x_hat", 264),
                 ("x_d_true", 264), ("post", 260), ("sigma2_t", 260), ("idx_hat", 258),
                 ("labels", 258)):
        assert _call(L, lib, **{k: v}) == -1, k
    assert _call(L, lib, llr=260, labels=256) == -1
    assert _call(L, lib, err=258, labels=256, x_d_true=256) == -1
    # outside the compiled kernel set
    for bad in (D(2, 5, 2, 5, 12, 4, 0, 0.01), D(2, 2, 9, 5, 12, 4, 0, 0.01),
                D(2, 3, 2, 5, 12, 64, 0, 0.01), D(2, 4, 4, 5, 12, 32, 0, 0.01)):
        assert _call(L, lib, dims=bad) == -2
    assert b"supported" in lib.sbce_strerror(-2)


def test_python_layer_argument_checks_without_gpu(sbce):
    import torch
    from importlib import import_module
    em = import_module(sbce.__name__ + ".em")
    # a non-square table has no default labelling when bits are asked for
    with pytest.raises(ValueError):
        em._detect_labels(8, None, True)
    assert em._detect_labels(8, None, False) is None
    assert np.array_equal(em._detect_labels(16, None, True), sbce.qam.gray_labeling(16))
    with pytest.raises(ValueError):
        em._detect_labels(4, [0, 1, 2, 2], True)
    assert em._detect_labels(8, np.arange(8)[::-1], True).dtype == np.int32
    if not torch.cuda.is_available():
        with pytest.raises(sbce.SbceUnavailable):
            sbce.detect_batch(np.zeros((1, 2, 1), complex), np.ones((1, 2, 1), complex),
                              np.array([1, -1], complex), np.ones((1, 1), complex), 0.1, 1,
                              want=("idx",))


# ------------------------------------------------------------------ sweep host logic
def test_sweep_routes_estimators_and_reduces_once(sbce, monkeypatch):
    sw = sbce.sweeps
    calls = {"em": [], "det": [], "allreduce": 0}

    def fake_em(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", partition_r=0, **kw):
        calls["em"].append((mode, partition_r, itera))
        # a fixed, mode-dependent estimate: theta0 pulled towards 0
        return {"theta": np.asarray(theta0) * (1.0 - 0.01 * (1 + len(mode)))}

    def det(*a, **kw):
        calls["det"].append(np.asarray(a[3]).copy())
        assert kw["want"] == () and kw["x_d_true"] is not None and kw["labels"] is not None
        return orc.oracle_detect_batch(*a, **kw)

    real = sw.Accumulators.allreduce

    def counting(self, dist=None, device=None):
        calls["allreduce"] += 1
        return real(self, dist, device)

    monkeypatch.setattr(sw, "em_batch", fake_em)
    monkeypatch.setattr(sw, "detect_batch", det)
    monkeypatch.setattr(sw.Accumulators, "allreduce", counting)
    kw = dict(SNR=(0, 15), T_d=12, T_p=6, N=4, n_rx=2, n_tx=2, itera=3, monte_iter=4, M=4, seed=3)
    ests = ("pilot", "soft", "pm", "genie")
    snr, ser, ber, nmse = sw.detection_vs_snr(estimators=ests, **kw)
    assert calls["allreduce"] == 1
    assert [c[0] for c in calls["em"]] == ["soft", "pm"] and calls["em"][1][1] == 1
    assert calls["em"][0][1] == 0 and all(c[2] == 3 for c in calls["em"])
    assert list(snr) == [0, 15] and set(ser) == set(ber) == set(nmse) == set(ests)
    # the same detector was fed h0, the estimates and h, over both SNR points' trials at once
    points, varns = sw.gen_snr(kw["SNR"], 12, 6, 4, 2, 2, 4, 4, 10.0, 3, True, 1.0)
    h0 = np.stack([t["h0"] for p in points for t in p])
    h = np.stack([t["h"] for p in points for t in p])
    assert len(calls["det"]) == 4
    assert np.array_equal(calls["det"][0], h0) and np.array_equal(calls["det"][3], h)
    assert np.array_equal(calls["det"][1], h0 * (1.0 - 0.01 * 5))
    assert np.all(nmse["genie"] == 0.0) and np.all(nmse["pilot"] > 0.0)
    # the extras are the restatement's counts, per SNR point
    cons, lab = sbce.qam.qam_constellation(4), sbce.qam.gray_labeling(4)
    for k, (trials, vn) in enumerate(zip(points, varns)):
        y = np.stack([t["Y_d"] for t in trials])
        psi = np.stack([t["Psi_d"].T for t in trials])
        x = np.stack([t["X_d"] for t in trials])
        for est, th in (("pilot", np.stack([t["h0"] for t in trials])),
                        ("genie", np.stack([t["h"] for t in trials]))):
            e = orc.detect_ref(y, psi, cons, th, vn * vn, 2, labels=lab, x_d_true=x)["err"]
            assert ser[est][k] == e[:, 0].sum() / (4 * 12 * 2)
            assert ber[est][k] == e[:, 1].sum() / (4 * 12 * 2 * 2)
    assert np.all(ser["genie"] <= ser["pilot"])
    # one call per SNR point gives the same curves
    snr2, ser2, ber2, nmse2 = sw.detection_vs_snr(estimators=ests, batch_snr=False, **kw)
    assert calls["allreduce"] == 2
    for e in ests:
        assert np.array_equal(ser[e], ser2[e]) and np.array_equal(ber[e], ber2[e])
        assert np.allclose(nmse[e], nmse2[e], rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        sw.detection_vs_snr(estimators=("pilot", "nonsense"), **kw)
