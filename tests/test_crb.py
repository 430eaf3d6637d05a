"""CPU tier of the Cramer-Rao bounds (sbce_crb): the NumPy oracle against an independent K x K
Fisher matrix and against a Monte-Carlo least-squares run, the C-ABI's validation (decided before
any HIP call, so it runs without a GPU) and the Python layer's additions."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import crb_oracle as orc

HEADER = os.path.join(ROOT, "include", "sbce.h")
# (n_tx, n_rx, P, T_p, T_d, M)
FISHER_SHAPES = [(1, 2, 8, 8, 30, 16), (2, 2, 4, 16, 12, 4), (2, 2, 17, 16, 40, 4), (2, 4, 8, 16, 40, 16)]


def _batch(sbce, shape, B, varn, seed):
    n_tx, n_rx, P, T_p, T_d, M = shape
    return sbce.signal_model.synthetic_batch(B, n_tx, n_rx, P - 1, T_p, T_d, M, varn, seed=seed,
                                             pinv="scipy")


@pytest.mark.parametrize("shape", FISHER_SHAPES)
def test_reduced_form_is_the_full_fisher_inverse(sbce, shape):
    """n_rx sigma2 tr(R^-1) and sigma2 (R^-1)_ll against the inverse of the K x K Fisher matrix built
    from the regressor matrices Z = u^T (x) I: two routes to one number, 1e-12 relative."""
    n_tx, n_rx = shape[:2]
    b = _batch(sbce, shape, 2, 0.3, 31)
    for i in range(2):
        red = orc.crb_reduced(b["u_p"][i], b["psi_d"][i], orc.genie_S(b["x_d"][i]), n_rx, 0.3)
        assert red["identifiable"]
        total, var = orc.crb_fisher(b["u_p"][i], b["psi_d"][i], b["x_d"][i], n_rx, 0.3)
        d_tot = abs(red["mse"] - total) / total
        d_var = np.abs(np.repeat(0.3 * red["diag_inv"], n_rx) - var).max() / var.max()
        print(f"{shape} trial {i}: total {d_tot:.2e} per-coefficient {d_var:.2e}")
        assert d_tot <= 1e-12 and d_var <= 1e-12


def test_least_squares_with_known_data_attains_the_bound(sbce):
    """Monte Carlo: 4000 noise draws on one (2,2,4,16,12,4-QAM) trial; the mean squared error of
    least squares with every symbol known is n_rx sigma2 tr(R^-1) to 4 standard errors."""
    shape, varn, draws = (2, 2, 4, 16, 12, 4), 0.3, 4000
    b = _batch(sbce, shape, 1, varn, 5)
    n_tx, n_rx, P = shape[:3]
    red = orc.crb_reduced(b["u_p"][0], b["psi_d"][0], orc.genie_S(b["x_d"][0]), n_rx, varn)
    u_d = np.einsum("tp,ta->tpa", b["psi_d"][0], b["x_d"][0]).reshape(shape[4], P * n_tx)
    U = np.concatenate([b["u_p"][0], u_d])                       # (T, L)
    clean = U @ b["h"][0].reshape(P * n_tx, n_rx)                # (T, n_rx)
    g = np.random.default_rng(1)
    pinv = np.linalg.pinv(U)
    err = np.empty(draws)
    for k in range(draws):
        n = np.sqrt(varn / 2) * (g.normal(size=clean.shape) + 1j * g.normal(size=clean.shape))
        err[k] = np.sum(np.abs(pinv @ n) ** 2)                   # theta_hat - theta = pinv(U) n
    mean, se = err.mean(), err.std(ddof=1) / np.sqrt(draws)
    print(f"least squares {mean:.5f} +- {se:.5f}, bound {red['mse']:.5f}, "
          f"{abs(mean - red['mse']) / se:.2f} standard errors")
    assert abs(red["mse"] - 0.16298) < 1e-5
    assert abs(mean - red["mse"]) <= 4 * se
    # the estimator itself on one draw: lstsq on the noisy observations is theta + pinv(U) n
    th = orc.ls_known(clean + n, U, n_rx)
    assert np.allclose(th - b["h"][0], (pinv @ n).reshape(-1), atol=1e-12)


def test_pivot_rule_of_the_oracle():
    g = np.random.default_rng(0)
    A = g.normal(size=(6, 9)) + 1j * g.normal(size=(6, 9))
    R = A @ np.conj(A.T)
    piv, ok = orc.chol_pivots(R)
    assert ok and np.allclose(piv, np.real(np.diag(np.linalg.cholesky(R))) ** 2)
    R2 = R.copy()
    R2[:, 4] = R2[:, 1]
    R2[4, :] = R2[1, :]                       # row / column 4 repeats 1: pivot 4 is rounding noise
    piv, ok = orc.chol_pivots(R2)
    assert not ok and np.isnan(piv[5]) and abs(piv[4]) <= 1e-14 * np.real(np.diag(R2)).max()
    S = np.zeros((3, 2, 2))
    out = orc.crb_reduced(np.zeros((0, 4)), np.ones((3, 2)), S, 2, 0.5)
    assert not out["identifiable"] and np.isinf(out["tr_inv"]) and np.all(np.isinf(out["diag_inv"]))


def _fields(struct):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", decl.strip()).group(1)
            for decl in body.split(";") if decl.strip()]


def test_header_exports_and_ctypes_agree(sbce):
    L = sbce._lib
    src = open(HEADER).read()
    assert int(re.search(r"#define SBCE_ABI_VERSION (\d+)", src).group(1)) == L.SBCE_ABI_VERSION == 7
    for name in ("sbce_crb_workspace_bytes", "sbce_crb"):
        assert name in L.EXPORTED
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert _fields("sbce_crb_opts") == [f for f, _ in L.CrbOpts._fields_]
    # offsets by the C rules: double, 6 pointers, size_t, int32 -- no padding before flags
    offs = [getattr(L.CrbOpts, f).offset for f, _ in L.CrbOpts._fields_]
    assert offs == [0, 8, 16, 24, 32, 40, 48, 56, 64] and ctypes.sizeof(L.CrbOpts) == 72


def _dims(L, batch=3, n_tx=2, n_psi=5, varn=0.5):
    return L.Dims(batch, n_tx, 2, n_psi, 6, 12, 4, 0, varn, 1.0)


def _ptrs(L, **over):
    vals = dict(y_d=256, y_p=256, psi_d=256, u_p=256, cons=256, theta=256, x_d_true=None, llf=None,
                h_true=None, iters_done=None, status=None, workspace=256,
                workspace_bytes=1 << 40, x_dest=None, x_sup=None, varn_t=None)
    vals.update(over)
    return L.Ptrs(*[vals[f] for f, _ in L.Ptrs._fields_])


def _opts(L, **over):
    vals = dict(sigma2=0.5, sigma2_t=None, tr_inv=256, diag_inv=None, mse=None, bound=None,
                scratch=256, scratch_bytes=1 << 40, flags=0)
    vals.update(over)
    return L.CrbOpts(*[vals[f] for f, _ in L.CrbOpts._fields_])


@pytest.mark.parametrize("ab", [False, True])
def test_validation_return_codes_without_gpu(sbce, ab):
    """Everything below is decided before any HIP call (this runs without a GPU), the same in both
    library variants.  An empty batch (B = 0) is a valid call that launches nothing."""
    L = sbce._lib
    lib = L.load_ab() if ab else L.load()
    d0 = _dims(L, batch=0)

    def crb(dims=d0, ptrs=None, opts=None, mom=256, null_opts=False):
        p = ptrs if ptrs is not None else _ptrs(L)
        o = opts if opts is not None else _opts(L)
        return lib.sbce_crb(ctypes.byref(dims), ctypes.byref(p), mom,
                            None if null_opts else ctypes.byref(o), None)

    n = ctypes.c_size_t(0)
    # the limit: L = n_psi n_tx <= 512 (the batched-panel regime)
    d512, d513 = _dims(L, n_tx=1, n_psi=512), _dims(L, n_tx=1, n_psi=513)
    assert lib.sbce_crb_workspace_bytes(ctypes.byref(d513), ctypes.byref(n)) == -2
    assert crb(dims=_dims(L, batch=0, n_tx=1, n_psi=513)) == -2
    assert lib.sbce_crb_workspace_bytes(ctypes.byref(d512), ctypes.byref(n)) == 0
    # 32 diagonal-tile inverses (16 x 16 complex128) and one theta (K = 1024) per trial
    assert n.value == 3 * 32 * 256 * 16 + 3 * 1024 * 16
    assert crb(dims=_dims(L, batch=0, n_tx=1, n_psi=512)) == 0
    assert lib.sbce_crb_workspace_bytes(None, ctypes.byref(n)) == -1
    assert lib.sbce_crb_workspace_bytes(ctypes.byref(d512), None) == -1
    # a valid call with nothing to do is accepted (so every refusal below is the named argument's)
    assert crb() == 0
    assert crb(ptrs=_ptrs(L, h_true=256), opts=_opts(L, bound=256, mse=256, diag_inv=256,
                                                     sigma2_t=256)) == 0
    assert crb(null_opts=True) == -1
    assert crb(opts=_opts(L, tr_inv=None)) == -1
    assert crb(opts=_opts(L, scratch=None)) == -1
    for k in ("tr_inv", "diag_inv", "mse", "sigma2_t"):
        assert crb(opts=_opts(L, **{k: 260})) == -1, k
    assert crb(ptrs=_ptrs(L, h_true=256), opts=_opts(L, bound=260)) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert crb(opts=_opts(L, sigma2=bad)) == -1, bad
    assert crb(opts=_opts(L, bound=256)) == -1                  # bound without h_true
    assert crb(opts=_opts(L, flags=1)) == -1
    assert crb(dims=_dims(L), opts=_opts(L, scratch_bytes=255)) == -4
    # sbce_mstep's own checks
    assert crb(mom=None) == -1
    for k in ("y_d", "y_p", "psi_d", "u_p", "cons", "theta", "workspace"):
        assert crb(ptrs=_ptrs(L, **{k: None})) == -1, k
    assert crb(dims=_dims(L), ptrs=_ptrs(L, workspace_bytes=16)) == -4
    assert crb(dims=_dims(L, varn=0.0)) == -1


def test_python_layer_additions(sbce):
    assert inspect.signature(sbce.sweeps.nmse_vs_snr).parameters["bounds"].default is False
    g = np.random.default_rng(3)
    x = g.normal(size=(2, 5, 3)) + 1j * g.normal(size=(2, 5, 3))
    m, S = sbce.genie_moments(x)
    assert m.shape == (2, 5, 3) and S.shape == (2, 5, 3, 3) and np.array_equal(m, x)
    for b in range(2):
        for t in range(5):
            assert np.array_equal(S[b, t], np.outer(x[b, t], np.conj(x[b, t])))
    assert np.array_equal(S, orc.genie_S(x))
    with pytest.raises(ValueError):
        sbce.crb_batch(None, None, np.ones((1, 4, 2)), np.ones((1, 3, 4)), np.ones(4), 2, 0.3,
                       kind="nonsense")
    with pytest.raises(ValueError):
        sbce.crb_batch(None, None, np.ones((1, 4, 2)), np.ones((1, 3, 4)), np.ones(4), 2, 0.3,
                       kind="genie")
    with pytest.raises(ValueError):
        sbce.crb_batch(None, None, np.ones((1, 4, 2)), np.ones((1, 3, 5)), np.ones(4), 2, 0.3,
                       kind="pilot")
