"""CPU tier of the noise-variance estimation (sbce_noise_var / sbce_em_noise): the NumPy
restatement against the brute-force expectation and the likelihood it must not decrease, the ABI
(header, exports, ctypes layouts), every validation return code without a GPU, the Python
argument checks, and the sweep's host logic with the device calls replaced."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import noise_oracle as orc
from oracle.em_reduced import aps_from_cons, estep_moments, heff

HEADER = os.path.join(ROOT, "include", "sbce.h")


def _trial(sbce, n_tx, n_rx, P, T_p, T_d, M, varn, seed):
    b = sbce.signal_model.synthetic_batch(1, n_tx, n_rx, P - 1, T_p, T_d, M, varn, seed=seed)
    return dict(Y_d=b["y_d"][0], Y_p=b["y_p"][0], U_p=b["u_p"][0], Psi=b["psi_d"][0].T,
                cons=b["cons"], theta0=b["theta0"][0], h=b["h"][0])


# ------------------------------------------------------------------ restatement
@pytest.mark.parametrize("shape", [(2, 2, 8, 16, 40, 4), (3, 5, 5, 12, 33, 4)])
def test_noise_var_ref_is_the_posterior_expectation(sbce, shape):
    """Q of the residual form = sum_t sum_j beta_{t,j} ||y_t - H_t x_j||^2 + the pilot residuals,
    with beta the soft posterior the moments came from."""
    n_tx, n_rx, P, T_p, T_d, M = shape
    d = _trial(sbce, *shape, 0.3, seed=11)
    varn = 0.7
    aps = aps_from_cons(d["cons"], n_tx)
    theta = d["theta0"] * (1.0 + 0.05j)              # any theta: the identity is algebraic
    m, S, _, _ = estep_moments(theta, d["Y_d"], d["Psi"], aps, varn, "soft", chunk=T_d)
    H = heff(theta, d["Psi"], n_tx, n_rx)
    dist = np.sum(np.abs(d["Y_d"][:, None, :] - np.einsum("tra,ja->tjr", H, aps)) ** 2, axis=2)
    beta = np.exp(-(dist - dist.min(axis=1, keepdims=True)) / varn ** 2)
    beta /= beta.sum(axis=1, keepdims=True)
    brute = np.sum(beta * dist) + np.sum(np.abs(d["Y_p"] - d["U_p"] @ theta.reshape(-1, n_rx)) ** 2)
    s2, Q, _ = orc.noise_var_ref(d["Y_d"], d["Y_p"], d["U_p"], d["Psi"], theta, m, S, parts=True)
    assert abs(Q - brute) <= 1e-12 * brute, (Q, brute)
    assert s2 == Q / (n_rx * (T_p + T_d))


@pytest.mark.parametrize("shape,start", [((2, 2, 8, 16, 40, 4), 1.0), ((2, 2, 8, 16, 40, 4), 0.1),
                                         ((1, 2, 8, 8, 30, 16), 3.0)])
def test_soft_em_noise_does_not_decrease_the_likelihood(sbce, shape, start):
    n_tx = shape[0]
    d = _trial(sbce, *shape, 0.3, seed=5)
    r = orc.em_noise_ref(d["Y_d"], d["Y_p"], d["U_p"], d["Psi"], d["cons"], start, 8, d["theta0"],
                         n_tx)
    ll = [orc.loglik_soft(d["Y_d"], d["Y_p"], d["U_p"], d["Psi"], d["cons"], d["theta0"], start, n_tx)]
    ll += [orc.loglik_soft(d["Y_d"], d["Y_p"], d["U_p"], d["Psi"], d["cons"], th, v, n_tx)
           for th, v in r["trace"]]
    assert len(ll) == 9
    for a, b in zip(ll[:-1], ll[1:]):
        assert b >= a - 1e-9 * abs(a), ll
    assert r["status"] == 0 and r["iters_done"] == 8 and r["varn"] == r["hist"][-1]


def test_restatement_rules():
    assert orc.apply_rules(np.nan, 10.0, 0.4, 1e-3) == (0.4, 64)
    assert orc.apply_rules(np.inf, 10.0, 0.4, 1e-3) == (0.4, 64)
    assert orc.apply_rules(1e-9, 10.0, 0.4, 1e-3) == (1e-3, 64)
    assert orc.apply_rules(2.5, 10.0, 0.4, 1e-3) == (0.5, 0)


# ------------------------------------------------------------------ ABI
def _fields(cname):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*;", body)


def test_header_exports_and_ctypes_agree(sbce):
    L = sbce._lib
    src = open(HEADER).read()
    assert int(re.search(r"#define SBCE_ABI_VERSION (\d+)", src).group(1)) == L.SBCE_ABI_VERSION == 7
    for name in ("sbce_noise_workspace_bytes", "sbce_noise_var", "sbce_em_noise"):
        assert name in L.EXPORTED
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert _fields("sbce_noise_opts") == [f for f, _ in L.NoiseOpts._fields_]
    assert "#define SBCE_STATUS_NOISE 64" in src and L.SBCE_STATUS_NOISE == 64
    assert sbce.em_batch_noise is not None and sbce.noise_var_batch is not None


def test_noise_struct_layout_matches_c(sbce, tmp_path):
    L = sbce._lib
    names = [f for f, _ in L.NoiseOpts._fields_]
    items = ["sizeof(sbce_noise_opts)"] + [f"offsetof(sbce_noise_opts, {f})" for f in names]
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
    assert out == [ctypes.sizeof(L.NoiseOpts)] + [getattr(L.NoiseOpts, f).offset for f in names]


def _dims(L, batch=3, varn=0.5):
    return L.Dims(batch, 2, 2, 5, 6, 12, 4, 0, varn, 1.0)


def _ptrs(L, **over):
    vals = dict(y_d=256, y_p=256, psi_d=256, u_p=256, cons=256, theta=256, x_d_true=None, llf=None,
                h_true=None, iters_done=None, status=None, workspace=256,
                workspace_bytes=1 << 40, x_dest=None, x_sup=None, varn_t=None)
    vals.update(over)
    return L.Ptrs(*[vals[f] for f, _ in L.Ptrs._fields_])


def _opts(L, **over):
    vals = dict(varn_est=256, varn_hist=None, scratch=256, scratch_bytes=1 << 30, varn_min=1e-6,
                flags=0)
    vals.update(over)
    return L.NoiseOpts(*[vals[f] for f, _ in L.NoiseOpts._fields_])


@pytest.mark.parametrize("ab", [False, True])
def test_validation_return_codes_without_gpu(sbce, ab):
    """Everything below is decided before any HIP call (this runs without a GPU), the same in both
    library variants."""
    L = sbce._lib
    lib = L.load_ab() if ab else L.load()
    d, d0 = _dims(L), _dims(L, batch=0)

    def em(dims=d, ptrs=None, opts=None, iters=0, mode=L.SBCE_ESTEP_SOFT, solve=L.SBCE_SOLVE_CHOL,
           null_opts=False):
        p = ptrs if ptrs is not None else _ptrs(L)
        o = opts if opts is not None else _opts(L)
        return lib.sbce_em_noise(ctypes.byref(dims), ctypes.byref(p), iters, mode, solve,
                                 None if null_opts else ctypes.byref(o), None)

    def nv(dims=d0, ptrs=None, opts=None, mom=256):
        p = ptrs if ptrs is not None else _ptrs(L, workspace=None, workspace_bytes=0, cons=None)
        o = opts if opts is not None else _opts(L)
        return lib.sbce_noise_var(ctypes.byref(dims), ctypes.byref(p), mom, ctypes.byref(o), None)

    # the scratch size: ceil((T_d + T_p) n_rx / 256) block sums per trial, 256-byte granules
    n = ctypes.c_size_t(0)
    assert lib.sbce_noise_workspace_bytes(ctypes.byref(d), ctypes.byref(n)) == 0 and n.value == 256
    big = L.Dims(40, 4, 4, 65, 16, 256, 4, 0, 0.5, 1.0)
    assert lib.sbce_noise_workspace_bytes(ctypes.byref(big), ctypes.byref(n)) == 0
    assert n.value == (40 * 5 * 8 + 255) // 256 * 256
    assert lib.sbce_noise_workspace_bytes(None, ctypes.byref(n)) == -1
    assert lib.sbce_noise_workspace_bytes(ctypes.byref(d), None) == -1
    # a valid call with nothing to do is accepted (so every refusal below is the named argument's)
    assert em() == 0 and nv() == 0
    for mode in (L.SBCE_ESTEP_HARD, L.SBCE_ESTEP_PM_SOFT, L.SBCE_ESTEP_ZF, L.SBCE_ESTEP_MMSE):
        dm = L.Dims(3, 2, 2, 5, 6, 12, 4, 1 if mode == L.SBCE_ESTEP_PM_SOFT else 0, 0.5, 1.0)
        assert em(dims=dm, mode=mode) == 0, mode
    for fn in (em, nv):
        assert fn(ptrs=_ptrs(L, x_sup=256)) == -1
        assert fn(ptrs=_ptrs(L, llf=256, x_d_true=256)) == -1
        assert fn(opts=_opts(L, varn_est=None)) == -1
        assert fn(opts=_opts(L, varn_est=260)) == -1
        assert fn(opts=_opts(L, varn_hist=260)) == -1
        assert fn(opts=_opts(L, scratch=None)) == -1
        assert fn(opts=_opts(L, scratch=260)) == -1
        for bad in (0.0, -1.0, float("nan")):
            assert fn(opts=_opts(L, varn_min=bad)) == -1, bad
        assert fn(opts=_opts(L, flags=1)) == -1
    assert em(null_opts=True) == -1
    assert em(opts=_opts(L, scratch_bytes=255)) == -4
    assert nv(dims=d, opts=_opts(L, scratch_bytes=255)) == -4
    assert em(mode=L.SBCE_ESTEP_GAUSS) == -2
    # sbce_em's own checks still hold
    assert em(iters=-1) == -1 and em(solve=7) == -1
    assert em(ptrs=_ptrs(L, workspace_bytes=16)) == -4
    assert em(ptrs=_ptrs(L, theta=None)) == -1
    # sbce_noise_var: required pointers and moments
    for k in ("y_d", "y_p", "psi_d", "u_p", "theta"):
        assert nv(ptrs=_ptrs(L, **{k: None})) == -1, k
        assert nv(ptrs=_ptrs(L, **{k: 264})) == -1, k
    assert nv(mom=None) == -1 and nv(mom=264) == -1
    assert nv(ptrs=_ptrs(L, varn_t=260)) == -1
    assert nv(dims=_dims(L, varn=0.0)) == -1


def test_python_layer_argument_checks_without_gpu(sbce):
    import torch
    z = np.zeros
    args = (z((1, 4, 2), complex), z((1, 2, 2), complex), np.ones((1, 4, 3), complex),
            np.ones((1, 2, 6), complex))
    cons = sbce.qam.qam_constellation(4)
    th = z((1, 12), complex)
    with pytest.raises(ValueError):
        sbce.em_batch_noise(*args, cons, 0.5, 3, th, mode="gauss")
    with pytest.raises(ValueError):
        sbce.em_batch_noise(*args, cons, 0.5, 3, th, varn_min=0.0)
    with pytest.raises(ValueError):
        sbce.em_batch_noise(*args, cons, 0.5, 0, th)
    with pytest.raises(ValueError):
        sbce.em_batch_noise(*args, cons, 0.5, 3, th, solve="qr")
    m, S = z((1, 4, 2), complex), z((1, 4, 2, 2), complex)
    with pytest.raises(ValueError):
        sbce.noise_var_batch(*args, th, m, S[:, :, :1])
    with pytest.raises(ValueError):
        sbce.noise_var_batch(*args, th, m, S, varn_min=-1.0)
    with pytest.raises(ValueError):
        sbce.noise_var_batch(args[0], args[1], args[2], np.ones((1, 2, 5), complex), th, m, S)
    if not torch.cuda.is_available():
        with pytest.raises(sbce.SbceUnavailable):
            sbce.em_batch_noise(*args, cons, 0.5, 3, th)
        with pytest.raises(sbce.SbceUnavailable):
            sbce.noise_var_batch(*args, th, m, S)


# ------------------------------------------------------------------ sweep host logic
def test_sweep_routes_three_runs_and_reduces_once(sbce, monkeypatch):
    sw = sbce.sweeps
    calls = {"em": [], "noise": [], "allreduce": 0}

    def fake_em(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", **kw):
        calls["em"].append((np.array(varn, dtype=float, ndmin=1).copy(), itera, mode))
        # the estimate moves from theta0 towards h with the parameter's size
        return {"theta": np.asarray(theta0) * (1.0 + 0.01 * np.array(varn, ndmin=1)[:, None])}

    def fake_noise(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", varn_min=1e-6,
                   **kw):
        calls["noise"].append((varn, itera, mode, varn_min))
        B = len(theta0)
        return {"theta": np.asarray(theta0) * 1.5, "sigma2": np.arange(1, B + 1, dtype=float)}

    real = sw.Accumulators.allreduce

    def counting(self, dist=None, device=None):
        calls["allreduce"] += 1
        return real(self, dist, device)

    monkeypatch.setattr(sw, "em_batch", fake_em)
    monkeypatch.setattr(sw, "em_batch_noise", fake_noise)
    monkeypatch.setattr(sw.Accumulators, "allreduce", counting)
    kw = dict(SNR=(0, 10), T_d=12, T_p=6, N=4, n_rx=2, n_tx=2, itera=4, monte_iter=3, M=4, seed=3,
              varn_assumed=2.0)
    snr, curves, ratio = sw.noise_est_vs_snr(**kw)
    assert calls["allreduce"] == 1
    assert list(snr) == [0, 10] and tuple(curves) == sw.NOISE_CURVES
    points, varns = sw.gen_snr(kw["SNR"], 12, 6, 4, 2, 2, 3, 4, 10.0, 3, True, 1.0)
    # one call per curve over both SNR points' trials: per-trial generating parameters, then the
    # assumed one, then the estimating run started from the assumed one
    assert len(calls["em"]) == 2 and len(calls["noise"]) == 1
    assert np.array_equal(calls["em"][0][0], np.repeat(varns, 3))
    assert np.array_equal(calls["em"][1][0], [2.0])
    assert calls["noise"][0] == (2.0, 4, "soft", 1e-6)
    assert all(c[1] == 4 and c[2] == "soft" for c in calls["em"])
    h0 = np.stack([t["h0"] for p in points for t in p])
    h = np.stack([t["h"] for p in points for t in p])
    for k in range(2):
        sl = slice(3 * k, 3 * k + 3)
        assert np.isclose(curves["known"][k], sw._nmse(h0[sl] * (1 + 0.01 * varns[k]), h[sl]).mean(),
                          rtol=1e-13, atol=0)
        assert np.isclose(curves["assumed"][k], sw._nmse(h0[sl] * 1.02, h[sl]).mean(), rtol=1e-13,
                          atol=0)
        assert np.isclose(curves["estimated"][k], sw._nmse(h0[sl] * 1.5, h[sl]).mean(), rtol=1e-13,
                          atol=0)
        assert np.isclose(ratio[k], np.mean(np.arange(3 * k + 1, 3 * k + 4) / varns[k]), rtol=1e-13,
                          atol=0)
    # one call per SNR point gives the same curves
    _, curves2, ratio2 = sw.noise_est_vs_snr(batch_snr=False, **kw)
    assert calls["allreduce"] == 2 and len(calls["noise"]) == 3
    for c in sw.NOISE_CURVES:
        assert np.allclose(curves[c], curves2[c], rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        sw.noise_est_vs_snr(varn_assumed=0.0, **{k: v for k, v in kw.items() if k != "varn_assumed"})
