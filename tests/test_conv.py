"""CPU tier of the log-likelihood readout and the truth-free convergence stop (sbce_loglik /
sbce_em_conv): the NumPy restatement's likelihood ascent and stop rules, the ABI (header, exports,
ctypes layouts), every validation return code without a GPU, and the Python argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import conv_oracle as orc
import noise_oracle as nzo

HEADER = os.path.join(ROOT, "include", "sbce.h")
S22 = (2, 2, 8, 16, 40, 4)


def _trial(sbce, shape, varn, seed, i=0, B=1):
    n_tx, n_rx, P, T_p, T_d, M = shape
    b = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, varn, seed=seed)
    return (b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, b["cons"]), b["theta0"][i]


# ------------------------------------------------------------------ restatement
@pytest.mark.parametrize("estimate", [False, True])
def test_restated_soft_loop_does_not_decrease_the_likelihood(sbce, estimate):
    """10 iterations of the restated SOFT loop, no stop possible: ll_l >= ll_{l-1} - 1e-9 |ll|,
    also from the start value, with and without the noise update."""
    args, th0 = _trial(sbce, S22, 0.3, seed=21)
    start = 1.0 if estimate else 0.3
    r = orc.em_conv_ref(*args, start, 10, th0, 2, min_iters=10, estimate_noise=estimate,
                        loglik=True)
    ll = [orc.loglik_ref(*args, th0, start, 2)] + list(r["ll_hist"])
    assert len(ll) == 11 and r["iters_done"] == 10
    for a, b in zip(ll[:-1], ll[1:]):
        assert b >= a - 1e-9 * abs(a), ll


def test_per_symbol_terms_sum_to_the_likelihood(sbce):
    args, th0 = _trial(sbce, (3, 5, 5, 12, 33, 4), 0.3, seed=11)
    Y_d, Y_p, U_p, Psi, cons = args
    for v in (0.01, 0.3, 30.0):
        sym = orc.loglik_sym_ref(Y_d, Psi, cons, th0, v, 3)
        ep = Y_p - U_p @ th0.reshape(-1, 5)
        pil = -np.sum(np.abs(ep) ** 2) / v ** 2 - Y_p.size * np.log(np.pi * v * v)
        ll = orc.loglik_ref(*args, th0, v, 3)
        A, A_t = orc.error_scale(*args, th0, v, 3)
        assert np.all(np.isfinite(sym)) and abs(sym.sum() + pil - ll) <= 1e-13 * A
        assert np.all(np.abs(sym) <= A_t) and abs(ll) <= A


def test_restated_stop_rules(sbce):
    """The theta rule stops no earlier than min_iters, freezes the histories, sets the bit; with no
    stop possible the loop is em_noise_ref's."""
    B = 4
    n_tx, n_rx, P, T_p, T_d, M = S22
    b = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, 0.3, seed=21)
    its = []
    for i in range(B):
        args = (b["y_d"][i], b["y_p"][i], b["u_p"][i], b["psi_d"][i].T, b["cons"])
        r = orc.em_conv_ref(*args, 0.3, 16, b["theta0"][i], 2)
        k = r["iters_done"]
        its.append(k)
        assert k >= 2
        if k < 16:
            assert r["status"] & orc.STATUS_CONVERGED
            assert r["delta"][-1] <= 1.0 and all(d > 1.0 for d in r["delta"][1:-1])
            assert np.all(r["dtheta_hist"][k - 1:] == r["dtheta_hist"][k - 1])
        hi = orc.em_conv_ref(*args, 0.3, 16, b["theta0"][i], 2, min_iters=9)
        assert hi["iters_done"] >= max(k, 9) or hi["iters_done"] == 16
    assert len(set(its)) >= 3, its
    args = (b["y_d"][0], b["y_p"][0], b["u_p"][0], b["psi_d"][0].T, b["cons"])
    free = orc.em_conv_ref(*args, 1.0, 5, b["theta0"][0], 2, min_iters=5, estimate_noise=True)
    ref = nzo.em_noise_ref(*args, 1.0, 5, b["theta0"][0], 2)
    assert np.array_equal(free["theta"], ref["theta"]) and np.array_equal(free["hist"], ref["hist"])
    # a NaN never stops a trial: the product-form comparison is false
    nan = float("nan")
    assert not (nan <= 1e-12 * nan)


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
    for name in ("sbce_loglik_workspace_bytes", "sbce_loglik", "sbce_conv_workspace_bytes",
                 "sbce_em_conv"):
        assert name in L.EXPORTED
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert _fields("sbce_conv_opts") == [f for f, _ in L.ConvOpts._fields_]
    assert "#define SBCE_STATUS_CONVERGED 128" in src and L.SBCE_STATUS_CONVERGED == 128
    assert sbce.em_batch_conv is not None and sbce.loglik_batch is not None
    assert sbce.sweeps.convergence_vs_snr is not None


def test_conv_struct_layout_matches_c(sbce, tmp_path):
    L = sbce._lib
    names = [f for f, _ in L.ConvOpts._fields_]
    items = ["sizeof(sbce_conv_opts)"] + [f"offsetof(sbce_conv_opts, {f})" for f in names]
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
    assert out == [ctypes.sizeof(L.ConvOpts)] + [getattr(L.ConvOpts, f).offset for f in names]


def _dims(L, batch=3, varn=0.5, n_tx=2, n_rx=2, m=4, pr=0):
    return L.Dims(batch, n_tx, n_rx, 5, 6, 12, m, pr, varn, 1.0)


def _ptrs(L, **over):
    vals = dict(y_d=256, y_p=256, psi_d=256, u_p=256, cons=256, theta=256, x_d_true=None, llf=None,
                h_true=None, iters_done=None, status=None, workspace=256,
                workspace_bytes=1 << 40, x_dest=None, x_sup=None, varn_t=None)
    vals.update(over)
    return L.Ptrs(*[vals[f] for f, _ in L.Ptrs._fields_])


def _conv(L, **over):
    vals = dict(tol_theta=1e-6, tol_ll=0.0, min_iters=2, flags=0, dtheta_hist=None, ll_hist=None,
                scratch=256, scratch_bytes=1 << 30)
    vals.update(over)
    return L.ConvOpts(*[vals[f] for f, _ in L.ConvOpts._fields_])


def _noise(L, **over):
    vals = dict(varn_est=256, varn_hist=None, scratch=256, scratch_bytes=1 << 30, varn_min=1e-6,
                flags=0)
    vals.update(over)
    return L.NoiseOpts(*[vals[f] for f, _ in L.NoiseOpts._fields_])


@pytest.mark.parametrize("ab", [False, True])
def test_validation_return_codes_without_gpu(sbce, ab):
    """Everything below is decided before any HIP call (this runs without a GPU), the same in both
    library variants.  batch = 0 / iters = 0 make a valid call a no-op."""
    L = sbce._lib
    lib = L.load_ab() if ab else L.load()
    d, d0 = _dims(L), _dims(L, batch=0)

    def em(dims=d, ptrs=None, cv=None, nz=None, iters=0, mode=L.SBCE_ESTEP_SOFT,
           solve=L.SBCE_SOLVE_CHOL, null_cv=False):
        p = ptrs if ptrs is not None else _ptrs(L)
        c = cv if cv is not None else _conv(L)
        return lib.sbce_em_conv(ctypes.byref(dims), ctypes.byref(p), iters, mode, solve,
                                ctypes.byref(nz) if nz is not None else None,
                                None if null_cv else ctypes.byref(c), None)

    def ll(dims=d0, ptrs=None, out=256, sym=None, scratch=256, nbytes=1 << 30):
        p = ptrs if ptrs is not None else _ptrs(L, workspace=None, workspace_bytes=0)
        return lib.sbce_loglik(ctypes.byref(dims), ctypes.byref(p), out, sym, scratch, nbytes, None)

    # scratch sizes in 256-byte granules: per-symbol terms [B][T_d], pilot block sums
    # [B][ceil(T_p n_rx / 256)]; the stop adds theta_prev [B][K] complex and the iteration's ll [B]
    n = ctypes.c_size_t(0)
    assert lib.sbce_loglik_workspace_bytes(ctypes.byref(d), ctypes.byref(n)) == 0
    assert n.value == 512 + 256                          # 3*12*8 = 288 -> 512, 3*1*8 = 24 -> 256
    big = L.Dims(40, 4, 4, 65, 160, 256, 4, 0, 0.5, 1.0)
    up = lambda v: (v + 255) // 256 * 256
    assert lib.sbce_loglik_workspace_bytes(ctypes.byref(big), ctypes.byref(n)) == 0
    need_ll = up(40 * 256 * 8) + up(40 * 3 * 8)
    assert n.value == need_ll
    assert lib.sbce_conv_workspace_bytes(ctypes.byref(big), 0, ctypes.byref(n)) == 0
    need_cv = up(40 * 65 * 16 * 16) + up(40 * 8)
    assert n.value == need_cv
    assert lib.sbce_conv_workspace_bytes(ctypes.byref(big), 1, ctypes.byref(n)) == 0
    assert n.value == need_cv + need_ll
    assert lib.sbce_loglik_workspace_bytes(None, ctypes.byref(n)) == -1
    assert lib.sbce_loglik_workspace_bytes(ctypes.byref(d), None) == -1
    assert lib.sbce_conv_workspace_bytes(None, 0, ctypes.byref(n)) == -1
    assert lib.sbce_conv_workspace_bytes(ctypes.byref(d), 0, None) == -1

    # ---- sbce_em_conv: a valid call with nothing to do is accepted, with and without the noise
    # estimate and the ll history, in every supported mode
    assert em() == 0 and em(nz=_noise(L)) == 0
    assert em(cv=_conv(L, ll_hist=256, dtheta_hist=256, tol_ll=1e-9)) == 0
    assert em(cv=_conv(L, tol_theta=0.0)) == 0
    for mode in (L.SBCE_ESTEP_HARD, L.SBCE_ESTEP_PM, L.SBCE_ESTEP_PM_SOFT, L.SBCE_ESTEP_ZF,
                 L.SBCE_ESTEP_MMSE):
        pr = 1 if mode in (L.SBCE_ESTEP_PM, L.SBCE_ESTEP_PM_SOFT) else 0
        assert em(dims=_dims(L, pr=pr), mode=mode) == 0, mode
    d88 = _dims(L, n_tx=8, n_rx=8, pr=1)                 # the theta rule: PM at n_tx = 8 too
    assert em(dims=d88, mode=L.SBCE_ESTEP_PM_SOFT) == 0
    # the point is to need no truth
    assert em(ptrs=_ptrs(L, h_true=256)) == -1
    assert em(ptrs=_ptrs(L, llf=256, x_d_true=256)) == -1
    assert em(ptrs=_ptrs(L, x_sup=256)) == -1
    assert em(null_cv=True) == -1
    for bad in (-1e-9, float("nan")):
        assert em(cv=_conv(L, tol_theta=bad)) == -1
        assert em(cv=_conv(L, tol_ll=bad, ll_hist=256)) == -1
    assert em(cv=_conv(L, tol_ll=1e-9)) == -1            # tol_ll > 0 requires ll_hist
    assert em(cv=_conv(L, min_iters=0)) == -1
    assert em(cv=_conv(L, flags=1)) == -1
    assert em(cv=_conv(L, dtheta_hist=260)) == -1
    assert em(cv=_conv(L, ll_hist=260)) == -1
    assert em(cv=_conv(L, scratch=None)) == -1
    assert em(cv=_conv(L, scratch=264)) == -1
    assert em(mode=L.SBCE_ESTEP_GAUSS) == -2
    # ll_hist beyond the log-likelihood's limits: n_tx > 4, J > 65536
    assert em(dims=d88, mode=L.SBCE_ESTEP_PM_SOFT, cv=_conv(L, ll_hist=256)) == -2
    d3x64 = _dims(L, n_tx=3, m=64, pr=1)                 # J = 262144
    assert em(dims=d3x64, mode=L.SBCE_ESTEP_PM_SOFT, cv=_conv(L, ll_hist=256)) == -2
    assert em(dims=d3x64, mode=L.SBCE_ESTEP_PM_SOFT) == 0
    # scratch: theta_prev 3*20*16 = 960 -> 1024, ll 256, log-likelihood 768
    assert em(cv=_conv(L, scratch_bytes=1279)) == -4
    assert em(cv=_conv(L, scratch_bytes=1280)) == 0
    assert em(cv=_conv(L, ll_hist=256, scratch_bytes=2047)) == -4
    assert em(cv=_conv(L, ll_hist=256, scratch_bytes=2048)) == 0
    # the chain's own checks still hold, the noise options' too
    assert em(iters=-1) == -1 and em(solve=7) == -1
    assert em(ptrs=_ptrs(L, workspace_bytes=16)) == -4
    assert em(ptrs=_ptrs(L, theta=None)) == -1
    assert em(nz=_noise(L, varn_est=None)) == -1
    assert em(nz=_noise(L, scratch_bytes=255)) == -4

    # ---- sbce_loglik
    assert ll() == 0 and ll(sym=256) == 0 and ll(ptrs=_ptrs(L, varn_t=256)) == 0
    assert ll(ptrs=_ptrs(L, h_true=256, llf=256, workspace=None)) == 0   # unused
    for k in ("y_d", "y_p", "psi_d", "u_p", "cons", "theta"):
        assert ll(ptrs=_ptrs(L, **{k: None})) == -1, k
        assert ll(ptrs=_ptrs(L, **{k: 264})) == -1, k
    assert ll(ptrs=_ptrs(L, x_sup=256)) == -1
    assert ll(ptrs=_ptrs(L, varn_t=260)) == -1
    assert ll(out=None) == -1 and ll(out=260) == -1 and ll(sym=260) == -1
    assert ll(scratch=None) == -1 and ll(scratch=260) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert ll(dims=_dims(L, batch=0, varn=bad)) == -1, bad
    assert lib.sbce_loglik(None, ctypes.byref(_ptrs(L)), 256, None, 256, 1 << 30, None) == -1
    assert lib.sbce_loglik(ctypes.byref(d0), None, 256, None, 256, 1 << 30, None) == -1
    assert ll(dims=_dims(L, batch=0, n_tx=5)) == -2
    assert ll(dims=L.Dims(0, 2, 9, 5, 6, 12, 4, 0, 0.5, 1.0)) == -1     # n_rx > 8: bad dims
    assert ll(dims=_dims(L, batch=0, n_tx=3, m=64)) == -2
    assert ll(dims=_dims(L, batch=0, n_tx=4, m=16)) == 0                 # J = 65536: supported
    assert ll(dims=d, nbytes=767) == -4


def test_python_layer_argument_checks_without_gpu(sbce):
    import torch
    z = np.zeros
    args = (z((1, 4, 2), complex), z((1, 2, 2), complex), np.ones((1, 4, 3), complex),
            np.ones((1, 2, 6), complex))
    cons = sbce.qam.qam_constellation(4)
    th = z((1, 12), complex)
    for kw in (dict(mode="gauss"), dict(tol_theta=-1.0), dict(tol_ll=-1.0), dict(tol_ll=1e-9),
               dict(min_iters=0), dict(solve="qr"), dict(varn_min=0.0)):
        with pytest.raises(ValueError):
            sbce.em_batch_conv(*args, cons, 0.5, 3, th, **kw)
    with pytest.raises(ValueError):
        sbce.em_batch_conv(*args, cons, 0.5, 0, th)
    with pytest.raises(ValueError):
        sbce.loglik_batch(*args, cons, th, 0.5, 3)       # u_p width is P * 2
    if not torch.cuda.is_available():
        with pytest.raises(sbce.SbceUnavailable):
            sbce.em_batch_conv(*args, cons, 0.5, 3, th)
        with pytest.raises(sbce.SbceUnavailable):
            sbce.loglik_batch(*args, cons, th, 0.5, 2)
