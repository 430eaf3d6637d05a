"""Drop-in EM estimators with the reference's own signatures, running on the
MI355X through libsbce.so (ctypes C-ABI, include/sbce.h).  PyTorch-ROCm is used
only for device buffers and the current HIP stream.

Reference operator -> entry point here:
  em(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial)
      "Proposed method/Proposed_method_NMSEvsTp.py":50-83 (also
      Proposed_method_NMSEvsTd.py:44-76, SNR/all_Detectors.py:242-274)   -> em()
  em_ml(...same...)            all_detectorsvsTd.py:135-173, SNR/all_Detectors.py:132-167
                                                                        -> em_ml()
  em(..., Z_d, ..., n_tx)      IterationsvsLLF.py:45-77  (returns theta, LLF)
                                                                        -> em_llf()
  em(...) with LLF             ML_detecctor.py:51-86 (reads the global Z_d)
                                                                        -> em_ml_llf(..., Z_d=)
  em(... no h_initial ...)     root Proposed_method_NMSEvsTp.py:43-69 (zero init)
                                                                        -> em_zero_init()
  em_pm(..., h, n_tx, partition_r, X_d, qamCons)
                               PM.py:47-116 (uniform list weights)      -> em_pm()
  em_pm(... no all_possibleSymbols ...)
                               PM_beta.py:42-112 (posterior list weights) -> em_pm_soft()
  em_zf / em_mmse(..., h_initial, h)
                               all_detectorsvsTd.py:98-133 / :54-96      -> em_zf(), em_mmse()
  (no reference counterpart)   the same argument list, soft per-stream ZF / MMSE posteriors
                               on the clean channel, n_tx up to 8   -> em_zf_soft(), em_mmse_soft()
  expectation propagation (EP), n_tx up to 8                        -> em_ep()
  EM_Gaussian_proposed(y_d, y_p, T_d, T_p, z_p, PsiTilde_td, varn, itera, H_initial, varx, n_tx)
                               MIMO_Gaussian_proposed.py:56-89 (Gaussian prior)
                                                                        -> EM_Gaussian_proposed()
  EM_approx(PsiTilde_tp, PsiTilde_td, x_p, Y_p, Y_d, Iterations, varn, G)
                               "Comparision/Comparision T_d vs NMSE.py":106-145 (semi-blind
                               Gaussian approximation, the comparator)   -> EM_approx()
                               batched: ``em_approx_batch`` (one sbce_approx_em call)
Batched form for sweeps / benchmark: ``em_batch`` (one sbce_em call for all trials).

Semantics kept from the reference: inputs are not mutated, theta is returned
as a fresh (K,1) complex128 array, the posterior exponent uses varn**2
(PMd/Proposed_method_NMSEvsTp.py:66) while the data were generated with noise
variance varn.  The reference's per-iteration ``print(norm(theta))`` is
available with ``verbose=True``.  Near-singular normal equations do not raise
(``np.linalg.solve`` only raises on an exactly zero LU pivot, which float
rounding essentially never produces): the device Cholesky drops a pivot at or below
1e-14 max diag R and flags the trial (``last_status``): theta stays finite and its
range-space part is lstsq's minimum-norm solution (where the reference's LU returns
rounding noise).  ``solve='lstsq'`` is np.linalg.lstsq of PM.py:108
(the minimum-norm solution with lstsq's default singular-value cut, include/sbce.h
SBCE_SOLVE_MINNORM): the reference's policy for rank-deficient normal equations and
the intended fallback of all_detectorsvsTd.py:238-241.  ``solve='drop'`` is the same
solve as 'chol' (kept for older callers).
"""
import ctypes

import numpy as np

from . import _lib
from .layout import cons_from_aps, u_from_zp, check_structure


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.SbceUnavailable("no HIP device visible: the sbce estimator has no CPU path")
    return torch


def _dev(torch, arr, dtype=None):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return torch.from_numpy(a).to("cuda", non_blocking=False)


_MODES = {"soft": _lib.SBCE_ESTEP_SOFT, "hard": _lib.SBCE_ESTEP_HARD, "pm": _lib.SBCE_ESTEP_PM,
          "pm_soft": _lib.SBCE_ESTEP_PM_SOFT, "zf": _lib.SBCE_ESTEP_ZF,
          "mmse": _lib.SBCE_ESTEP_MMSE, "gauss": _lib.SBCE_ESTEP_GAUSS,
          "mmse_soft": _lib.SBCE_ESTEP_MMSE_SOFT, "zf_soft": _lib.SBCE_ESTEP_ZF_SOFT,
          "ep": _lib.SBCE_ESTEP_EP}
_SOLVES = {"chol": _lib.SBCE_SOLVE_CHOL, "drop": _lib.SBCE_SOLVE_CHOL_DROP,
           "lstsq": _lib.SBCE_SOLVE_MINNORM}


def _mode_word(mode, partition_r, ep_passes):
    """dims.partition_r of a call: the PM list parameter, or for mode "ep" the pass count
    (include/sbce.h SBCE_ESTEP_EP: None / 0 = the default 5, else 1..16)."""
    if mode != "ep":
        if ep_passes is not None:
            raise ValueError("ep_passes needs mode 'ep'")
        return int(partition_r)
    n = 0 if ep_passes is None else int(ep_passes)
    if not 0 <= n <= _lib.SBCE_EP_MAX_PASSES:
        raise ValueError(f"ep_passes must be 0 (the default) .. {_lib.SBCE_EP_MAX_PASSES}")
    return n


def _varn_arg(torch, varn, B):
    """(dims.varn, per-trial device tensor or None) for a scalar or (B,) noise variance."""
    if np.ndim(varn) == 0 and not (isinstance(varn, torch.Tensor) and varn.dim() > 0):
        v = float(varn)
        if not v > 0:
            raise ValueError("varn must be > 0")
        return v, None
    v = np.ascontiguousarray(varn.cpu().numpy() if isinstance(varn, torch.Tensor) else varn,
                             dtype=np.float64).reshape(-1)
    if v.size != B:
        raise ValueError(f"per-trial varn has {v.size} entries, batch is {B}")
    if not np.all(v > 0):
        raise ValueError("varn must be > 0")
    return float(v[0]), torch.from_numpy(v).to("cuda")


def _cdev(torch, x):
    """An input as a contiguous CUDA tensor: None stays None, a tensor is moved if it is not on
    the device (a contiguous CUDA tensor is used in place), an array becomes complex128."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return (x if x.is_cuda else x.to("cuda")).contiguous()
    return _dev(torch, x, np.complex128)


def _ptrs(t_p, **fields):
    """_lib.Ptrs by field name: a tensor gives its data_ptr(), None (or a field left out) is
    null, ``workspace`` also sets workspace_bytes; an unknown name raises TypeError.
    T_p == 0 (superimposed protocol, stand-alone E-step): an empty tensor's data_ptr() is 0,
    which the ABI rejects; the pilot buffers are never read then, so y_d stands in for both."""
    unknown = set(fields) - {f for f, _ in _lib.Ptrs._fields_}
    if unknown:                 # ctypes would take any keyword as a plain attribute
        raise TypeError(f"sbce_ptrs has no field {sorted(unknown)}")
    if not t_p:
        fields["y_p"] = fields["u_p"] = fields["y_d"]
    if fields.get("workspace") is not None:
        fields["workspace_bytes"] = fields["workspace"].numel()
    return _lib.Ptrs(**{k: v.data_ptr() if hasattr(v, "data_ptr") else v
                        for k, v in fields.items() if v is not None})


def _scratch(torch, query, what, *args):
    """A device scratch buffer of the size a sbce_*_workspace_bytes entry point reports."""
    nb = ctypes.c_size_t(0)
    _lib.check(query(*args, ctypes.byref(nb)), what)
    return torch.empty(max(nb.value, 16), dtype=torch.uint8, device="cuda")


class _Staged:
    """One problem on the device: the six input tensors, Dims, workspace, status and iters_done.

    check: the name of the theta argument in the shape errors of the batched entry points; None
    (the diagnostic stages) leaves every validation to the library.  clone: theta is a private
    copy of the input (theta0 keeps the input).  workspace: False for none, else the sbce_em
    workspace for the SBCE_SOLVE_* mode ``solve`` (None: for every mode)."""

    def __init__(self, torch, y_d, y_p, psi_d, u_p, cons, theta, varn, partition_r=0, varx=1.0,
                 solve=None, check=None, clone=False, workspace=True):
        self.y_d, self.y_p, self.psi_d, self.u_p, self.cons, self.theta0 = (
            _cdev(torch, x) for x in (y_d, y_p, psi_d, u_p, cons, theta))
        self.theta = self.theta0.clone() if clone else self.theta0
        B, T_d, n_rx = self.y_d.shape
        T_p, P, L = self.y_p.shape[1], self.psi_d.shape[2], self.u_p.shape[2]
        self.B, self.T_d, self.n_rx, self.T_p, self.P = B, T_d, n_rx, T_p, P
        if check and L % P:
            raise ValueError("u_p width must be P*n_tx")
        self.n_tx, self.M = L // P, self.cons.shape[0]
        if check and self.theta.shape != (B, L * n_rx):
            raise ValueError(f"{check} shape {tuple(self.theta.shape)} != {(B, L * n_rx)}")
        self.varn, self.varn_t = _varn_arg(torch, varn, B) if check else (float(varn), None)
        self.dims = _lib.Dims(B, self.n_tx, n_rx, P, T_p, T_d, self.M, int(partition_r), self.varn,
                              float(varx))
        self.ws = (torch.empty(max(_lib.workspace_bytes(self.dims, solve), 16), dtype=torch.uint8,
                               device="cuda") if workspace else None)
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.iters_done = torch.zeros(B, dtype=torch.int32, device="cuda")

    def ptrs(self, rows=slice(None), ws=None, **per_trial):
        """sbce_ptrs of the trials ``rows`` (a slice; default: all) with the workspace ``ws``
        (default: the problem's own); per_trial: further batch-major tensors by field name
        (x_d_true, llf, h_true, x_dest, x_sup), None for absent."""
        per_trial.update(y_d=self.y_d, y_p=self.y_p, psi_d=self.psi_d, u_p=self.u_p,
                         theta=self.theta, iters_done=self.iters_done, status=self.status,
                         varn_t=self.varn_t)
        views = {k: v[rows] for k, v in per_trial.items() if v is not None}
        return _ptrs(self.T_p, cons=self.cons, workspace=self.ws if ws is None else ws, **views)


def _result(torch, out, return_device):
    """The result dict as it is (device tensors), or synchronised and copied to numpy."""
    if return_device:
        return out
    torch.cuda.current_stream().synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _prior_arg(torch, prior_llr, labels, B, T_d, n_tx, M, mode="ep"):
    """A-priori bit L-values of a call (include/sbce.h sbce_prior_opts): (la, labels) as device
    tensors -- la (B,T_d,n_tx,log2 M) float64, log(P(bit = 0) / P(bit = 1)), NaN / inf allowed --
    or (None, None) without a prior.  labels=None: the package's Gray labelling."""
    if prior_llr is None:
        return None, None
    if mode != "ep":
        raise ValueError("prior_llr needs the expectation-propagation mode / kind 'ep'")
    lgM = max(int(M - 1).bit_length(), 1)
    if isinstance(prior_llr, torch.Tensor):
        la = prior_llr.to(device="cuda", dtype=torch.float64).contiguous()
    else:
        la = _dev(torch, prior_llr, np.float64)
    if tuple(la.shape) != (B, T_d, n_tx, lgM):
        raise ValueError(f"prior_llr shape {tuple(la.shape)} != {(B, T_d, n_tx, lgM)}")
    if isinstance(labels, torch.Tensor):
        return la, labels
    return la, torch.from_numpy(_detect_labels(M, labels, True)).to("cuda")


class _Prior:
    """sbce_prior_opts of a call and the tensors it points to (kept alive with it)."""

    def __init__(self, la, lab):
        self.la, self.lab = la, lab
        self.opts = _lib.PriorOpts(la.data_ptr(), lab.data_ptr(), 0) if la is not None else None

    def ref(self):
        return ctypes.byref(self.opts) if self.opts is not None else None


def em_batch(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", x_d_true=None,
             h_true=None, solve="chol", return_device=False, partition_r=0,
             return_decisions=False, x_sup=None, varx=1.0, ep_passes=None, prior_llr=None,
             labels=None):
    """Run ``itera`` EM iterations on a batch of independent trials.

    Array layouts (complex128, batch-major, include/sbce.h):
      y_d (B,T_d,n_rx), y_p (B,T_p,n_rx), psi_d (B,T_d,P) [RIS phases per data
      symbol, row 0 of the reference's PsiTilde_td = direct path], u_p (B,T_p,L),
      cons (M,), theta0 (B,K) with K = P*n_tx*n_rx.
    Optional: x_d_true (B,T_d,n_tx) -> per-iteration LLF (IterationsvsLLF.py:76);
    h_true (B,K) -> the reference's oracle early stop (PM.py:110-112).
    mode: "soft" | "hard" | "pm" | "pm_soft" | "zf" | "mmse" | "mmse_soft" | "zf_soft" | "ep";
    partition_r selects the PM list size.  "mmse_soft" / "zf_soft": the soft E-step for up to 8
    streams -- per-stream MMSE / ZF equalisation on the clean channel and a Gaussian soft demapper
    (detect_linear_batch's moments, include/sbce.h SBCE_ESTEP_MMSE_SOFT); "zf_soft" needs
    n_rx >= n_tx, neither takes x_sup or return_decisions.  "ep": expectation propagation
    (SBCE_ESTEP_EP), ``ep_passes`` passes (None: 5; 1..16) of the "mmse_soft" solve, each with the
    demapper's per-stream means and variances of the pass before as the prior; limits as
    "mmse_soft".  return_decisions (hard modes): x_dest (B,T_d,n_tx), the last E-step's
    decisions (SER/log_max_SER.py:77-78).  x_sup (B,T_d,n_tx): pilot symbols superimposed
    on the data (Parallel/ParallelProtocol_Tp.py:63-86), soft/hard modes.  mode "gauss":
    Gaussian-prior EM (MIMO_Gaussian_proposed.py:56-89) with prior variance parameter varx;
    psi_d then has P = N rows (no direct path), cons is ignored, theta is the reduced
    channel (gauss_expand_batch gives the reference's n_rx x Q matrix).
    prior_llr (B,T_d,n_tx,log2 M) (mode "ep" only): a-priori bit L-values log(P(bit = 0) /
    P(bit = 1)) of the data symbols, e.g. a decoder's feedback or qam.prior_llr_known's for known
    symbols (sbce_em_prior: soft-input EP, the moments are a-posteriori); labels: the labelling
    they refer to (None: Gray, as detect_batch).
    Inputs may be numpy arrays or CUDA complex128 tensors (used in place).  varn may be one
    value or one per trial ((B,) array: the trials of several SNR points in one call, include/
    sbce.h sbce_ptrs.varn_t; each trial's result is that of a call with its own varn).
    Returns dict(theta (B,K), llf (B,itera) or None, status (B,), iters_done (B,)).
    """
    torch = _torch()
    lib = _lib.load()
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta0, varn,
                 _mode_word(mode, partition_r, ep_passes), varx,
                 solve=_SOLVES[solve], check="theta0", clone=True)
    Xd, Ht, Xs = (_cdev(torch, x) for x in (x_d_true, h_true, x_sup))
    llf = (torch.zeros((st.B, max(itera, 1)), dtype=torch.float64, device="cuda")
           if Xd is not None else None)
    xdest = (torch.zeros((st.B, st.T_d, st.n_tx), dtype=torch.complex128, device="cuda")
             if return_decisions else None)
    ptrs = st.ptrs(x_d_true=Xd, llf=llf, h_true=Ht, x_dest=xdest, x_sup=Xs)
    stream = torch.cuda.current_stream().cuda_stream
    pr = _Prior(*_prior_arg(torch, prior_llr, labels, st.B, st.T_d, st.n_tx, st.M, mode))
    if pr.opts is None:
        _lib.check(lib.sbce_em(st.dims, ptrs, int(itera), _MODES[mode], _SOLVES[solve], stream),
                   "sbce_em")
    else:
        _lib.check(lib.sbce_em_prior(st.dims, ptrs, int(itera), _MODES[mode], _SOLVES[solve],
                                     pr.ref(), None, None, stream), "sbce_em_prior")
    out = dict(theta=st.theta, llf=llf, status=st.status, iters_done=st.iters_done)
    if xdest is not None:
        out["x_dest"] = xdest
    return _result(torch, out, return_device)


_NOISE_MODES = ("soft", "hard", "pm", "pm_soft", "zf", "mmse", "mmse_soft", "zf_soft", "ep")


def _noise_checks(mode, varn_min):
    """Argument checks of the noise-estimating calls (made before the device is touched)."""
    if mode not in _NOISE_MODES:
        raise ValueError(f"noise estimation supports the modes {_NOISE_MODES}, not {mode!r}")
    vmin = float(varn_min)
    if not vmin > 0:
        raise ValueError("varn_min must be > 0")
    return vmin


def _noise_opts(torch, lib, st, vmin, iters=0):
    """sbce_noise_opts for the staged problem: (opts, varn_est (B,), varn_hist (B,iters) or None
    when iters == 0, the scratch buffer the caller keeps alive)."""
    scratch = _scratch(torch, lib.sbce_noise_workspace_bytes, "sbce_noise_workspace_bytes",
                       ctypes.byref(st.dims))
    est = torch.zeros(st.B, dtype=torch.float64, device="cuda")
    hist = torch.zeros((st.B, iters), dtype=torch.float64, device="cuda") if iters else None
    opts = _lib.NoiseOpts(est.data_ptr(), hist.data_ptr() if iters else None, scratch.data_ptr(),
                          scratch.numel(), vmin, 0)
    return opts, est, hist, scratch


def noise_var_batch(y_d, y_p, psi_d, u_p, theta, m, S, varn_min=1e-6, return_status=False):
    """One noise-variance update per trial (sbce_noise_var, csrc/noise.hip) from a channel estimate
    and posterior moments: sigma^2 = Q / (n_rx (T_p + T_d)),
    Q = sum_p ||y_p - H_c u_p||^2 + sum_t (||y_t - H_t m_t||^2 + tr(H_t (S_t - m_t m_t^H) H_t^H)).
    Layouts as em_batch; theta (B,K), m (B,T_d,n_tx), S (B,T_d,n_tx,n_tx) (estep_batch's outputs).
    Returns sigma^2 (B,) float64 [, status (B,): SBCE_STATUS_NOISE where sigma^2 < varn_min^2 and
    varn_min^2 is returned]."""
    vmin = _noise_checks("soft", varn_min)
    B, T_d, n_rx = np.shape(y_d)
    n_tx = np.shape(m)[2]
    if np.shape(S) != (B, T_d, n_tx, n_tx) or np.shape(m) != (B, T_d, n_tx):
        raise ValueError("noise_var_batch: m must be (B,T_d,n_tx) and S (B,T_d,n_tx,n_tx)")
    if np.shape(u_p)[2] != np.shape(psi_d)[2] * n_tx:
        raise ValueError("u_p width must be P*n_tx")
    torch = _torch()
    lib = _lib.load()
    st = _Staged(torch, y_d, y_p, psi_d, u_p, np.ones(2, dtype=complex), theta, 1.0,
                 workspace=False)
    mom = _dev(torch, np.concatenate([np.asarray(m).reshape(B, T_d, n_tx),
                                      np.asarray(S).reshape(B, T_d, n_tx * n_tx)], axis=2),
               np.complex128)
    opts, est, _, scratch = _noise_opts(torch, lib, st, vmin)
    _lib.check(lib.sbce_noise_var(st.dims, st.ptrs(), mom.data_ptr(), opts,
                                  torch.cuda.current_stream().cuda_stream), "sbce_noise_var")
    torch.cuda.current_stream().synchronize()
    v = est.cpu().numpy()
    return (v * v, st.status.cpu().numpy()) if return_status else v * v


def em_batch_noise(y_d, y_p, psi_d, u_p, cons, varn, itera, theta0, mode="soft", solve="chol",
                   partition_r=0, h_true=None, varn_min=1e-6, return_device=False, ep_passes=None,
                   prior_llr=None, labels=None):
    """em_batch with the noise parameter unknown (sbce_em_noise): it is estimated per trial beside
    theta, on the device, inside the iteration chain -- per iteration E-step, M-step, noise update
    (csrc/noise.hip), oracle early stop.  ``varn`` (one value or (B,)) is only the START of the
    parameter; the posterior of every E-step divides by the current estimate squared, sigma^2.
    mode: "soft" | "hard" | "pm" | "pm_soft" | "zf" | "mmse" | "mmse_soft" | "zf_soft" | "ep"
    (with ``ep_passes``, ``prior_llr`` and ``labels``, as em_batch).  varn_min:
    floor of the parameter (a trial that reaches it has SBCE_STATUS_NOISE set and varn == varn_min exactly).
    Returns dict(theta (B,K), varn (B,) the parameter after each trial's last update, sigma2 =
    varn**2, hist (B,itera) the parameter after each iteration (a stopped trial's later entries
    hold its last value), status (B,), iters_done (B,)).
    ``detect_batch(..., varn=res["varn"], noise="em")`` demaps with the estimated variance."""
    vmin = _noise_checks(mode, varn_min)
    if solve not in _SOLVES:
        raise ValueError(f"unknown solve {solve!r}")
    if int(itera) < 1:
        raise ValueError("itera must be >= 1")
    torch = _torch()
    lib = _lib.load()
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta0, varn,
                 _mode_word(mode, partition_r, ep_passes),
                 solve=_SOLVES[solve], check="theta0", clone=True)
    opts, est, hist, scratch = _noise_opts(torch, lib, st, vmin, int(itera))
    Ht = _cdev(torch, h_true)
    pr = _Prior(*_prior_arg(torch, prior_llr, labels, st.B, st.T_d, st.n_tx, st.M, mode))
    stream = torch.cuda.current_stream().cuda_stream
    if pr.opts is None:
        _lib.check(lib.sbce_em_noise(st.dims, st.ptrs(h_true=Ht), int(itera), _MODES[mode],
                                     _SOLVES[solve], opts, stream), "sbce_em_noise")
    else:
        _lib.check(lib.sbce_em_prior(st.dims, st.ptrs(h_true=Ht), int(itera), _MODES[mode],
                                     _SOLVES[solve], pr.ref(), ctypes.byref(opts), None, stream),
                   "sbce_em_prior")
    out = dict(theta=st.theta, varn=est, sigma2=est * est, hist=hist, status=st.status,
               iters_done=st.iters_done)
    return _result(torch, out, return_device)


def loglik_batch(y_d, y_p, psi_d, u_p, cons, theta, varn, n_tx, per_symbol=False):
    """Observed-data log-likelihood of every trial (sbce_loglik, csrc/loglik.hip) at a channel
    estimate theta (B,K) and the noise parameter varn (one value or (B,); sigma^2 = varn**2, the
    E-step's denominator) under uniform symbols: the pilots' Gaussian terms plus, per data symbol,
    log (1/J) sum_j CN(y_t; H_t x_j, sigma^2 I) over the J = M**n_tx hypotheses -- the quantity
    the soft EM ascends.  Layouts as em_batch; needs no ground truth.
    Returns ll (B,) float64 [, ll_sym (B,T_d): the data symbols' terms]."""
    if np.shape(u_p)[2] != np.shape(psi_d)[2] * int(n_tx):
        raise ValueError("u_p width must be P*n_tx")
    torch = _torch()
    lib = _lib.load()
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta, varn, check="theta", workspace=False)
    ll = torch.zeros(st.B, dtype=torch.float64, device="cuda")
    sym = torch.zeros((st.B, st.T_d), dtype=torch.float64, device="cuda") if per_symbol else None
    scratch = _scratch(torch, lib.sbce_loglik_workspace_bytes, "sbce_loglik_workspace_bytes",
                       ctypes.byref(st.dims))
    _lib.check(lib.sbce_loglik(st.dims, st.ptrs(), ll.data_ptr(),
                               sym.data_ptr() if per_symbol else None,
                               scratch.data_ptr(), scratch.numel(),
                               torch.cuda.current_stream().cuda_stream), "sbce_loglik")
    torch.cuda.current_stream().synchronize()
    return (ll.cpu().numpy(), sym.cpu().numpy()) if per_symbol else ll.cpu().numpy()


def em_batch_conv(y_d, y_p, psi_d, u_p, cons, varn, max_iters, theta0, tol_theta=1e-6, tol_ll=0.0,
                  min_iters=2, estimate_noise=False, varn_min=1e-6, loglik=False, mode="soft",
                  partition_r=0, solve="chol", return_device=False, ep_passes=None,
                  prior_llr=None, labels=None):
    """em_batch with a per-trial stop that needs no ground truth (sbce_em_conv): a trial stops
    after iteration l (at least min_iters performed) when ||theta_l - theta_{l-1}|| <= tol_theta
    ||theta_l|| (theta_{-1} = theta0), or -- tol_ll > 0, which needs loglik=True -- when its
    observed-data log-likelihood rose by at most tol_ll |ll_l|.  A stopped trial is frozen and
    skipped by every later launch.  estimate_noise: the noise parameter is estimated beside theta
    as in em_batch_noise (``varn`` is then only its start).  loglik=True records the
    log-likelihood after every iteration (one sbce_loglik pass each: a diagnostic, soft-EM shapes
    with n_tx <= 4 and M**n_tx <= 65536 only).  mode: as em_batch_noise ("mmse_soft" / "zf_soft" / "ep"
    included: the theta rule works at every n_tx, loglik=True keeps its n_tx <= 4 limit).
    prior_llr / labels: as em_batch (mode "ep"; not together with loglik=True).
    Returns dict(theta (B,K), iters_done (B,), status (B,) with SBCE_STATUS_CONVERGED where a rule
    stopped the trial, dtheta_hist (B,max_iters) the relative step after each iteration, ll_hist
    (B,max_iters) or None, varn (B,) the parameter each trial ended with, sigma2 = varn**2, hist
    (B,max_iters) the parameter's history or None); a stopped trial's later history entries hold
    its last value."""
    if mode not in _NOISE_MODES:
        raise ValueError(f"the convergence stop supports the modes {_NOISE_MODES}, not {mode!r}")
    if solve not in _SOLVES:
        raise ValueError(f"unknown solve {solve!r}")
    iters, mi = int(max_iters), int(min_iters)
    if iters < 1 or mi < 1:
        raise ValueError("max_iters and min_iters must be >= 1")
    tt, tl = float(tol_theta), float(tol_ll)
    if not tt >= 0 or not tl >= 0:
        raise ValueError("tol_theta and tol_ll must be >= 0")
    if tl > 0 and not loglik:
        raise ValueError("tol_ll > 0 needs loglik=True")
    vmin = _noise_checks(mode, varn_min)
    torch = _torch()
    lib = _lib.load()
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta0, varn,
                 _mode_word(mode, partition_r, ep_passes),
                 solve=_SOLVES[solve], check="theta0", clone=True)
    B = st.B
    dth = torch.zeros((B, iters), dtype=torch.float64, device="cuda")
    llh = torch.zeros((B, iters), dtype=torch.float64, device="cuda") if loglik else None
    cscratch = _scratch(torch, lib.sbce_conv_workspace_bytes, "sbce_conv_workspace_bytes",
                        ctypes.byref(st.dims), 1 if loglik else 0)
    cv = _lib.ConvOpts(tt, tl, mi, 0, dth.data_ptr(), llh.data_ptr() if loglik else None,
                       cscratch.data_ptr(), cscratch.numel())
    nz, hist = None, None
    if estimate_noise:
        nz, est, hist, nscratch = _noise_opts(torch, lib, st, vmin, iters)
    elif st.varn_t is not None:
        est = st.varn_t
    else:
        est = torch.full((B,), st.varn, dtype=torch.float64, device="cuda")
    pr = _Prior(*_prior_arg(torch, prior_llr, labels, st.B, st.T_d, st.n_tx, st.M, mode))
    nzr = ctypes.byref(nz) if nz is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    if pr.opts is None:
        _lib.check(lib.sbce_em_conv(st.dims, st.ptrs(), iters, _MODES[mode], _SOLVES[solve], nzr,
                                    ctypes.byref(cv), stream), "sbce_em_conv")
    else:
        _lib.check(lib.sbce_em_prior(st.dims, st.ptrs(), iters, _MODES[mode], _SOLVES[solve],
                                     pr.ref(), nzr, ctypes.byref(cv), stream), "sbce_em_prior")
    out = dict(theta=st.theta, iters_done=st.iters_done, status=st.status, dtheta_hist=dth,
               ll_hist=llh, varn=est, sigma2=est * est, hist=hist)
    return _result(torch, out, return_device)


def _prepare_single(Y_d, Y_p, Z_p, PsiTilde_td, all_possibleSymbols, M, h_initial, n_tx=None,
                    cons=None):
    n_rx = np.asarray(Y_d[0]).shape[0]
    aps = None if all_possibleSymbols is None else np.asarray(all_possibleSymbols)
    if aps is not None:
        n_tx = aps.shape[1]
        cons = cons_from_aps(aps, int(M)) if cons is None else np.asarray(cons, dtype=complex)
    else:
        cons = np.asarray(cons, dtype=complex).reshape(-1)
    Psi = np.asarray(PsiTilde_td)
    P = Psi.shape[0]
    K = P * n_tx * n_rx
    U_p = u_from_zp(Z_p, n_rx) if len(Z_p) else np.zeros((0, P * n_tx), dtype=complex)
    check_structure(Z_p, U_p, n_rx, aps, cons, K)
    y_d = np.stack([np.asarray(y).reshape(-1) for y in Y_d])[None]
    y_p = (np.stack([np.asarray(y).reshape(-1) for y in Y_p])[None] if len(Y_p)
           else np.zeros((1, 0, n_rx), dtype=complex))
    th0 = (np.zeros(K, dtype=complex) if h_initial is None
           else np.asarray(h_initial, dtype=complex).reshape(-1))
    if th0.size != K:
        raise ValueError(f"h_initial has {th0.size} entries, expected K={K}")
    return dict(y_d=y_d, y_p=y_p, psi_d=Psi.T[None], u_p=U_p[None], cons=cons,
                theta0=th0[None], n_tx=n_tx, n_rx=n_rx, P=P, K=K)


last_status = 0


def _finish(res, verbose, itera):
    global last_status
    last_status = int(res["status"][0])
    th = res["theta"][0].reshape(-1, 1)
    if verbose:
        print(np.linalg.norm(th))
    return th


def em(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial,
       verbose=False, solve="chol"):
    """Exact soft EM (PMd/Proposed_method_NMSEvsTp.py:50-83) on the GPU."""
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d],
                        all_possibleSymbols, M, h_initial)
    if verbose:
        print("inital theta", np.linalg.norm(d["theta0"]))
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode="soft", solve=solve)
    return _finish(res, verbose, itera)


def em_ml(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial,
          verbose=False, solve="chol"):
    """Hard-ML ("log-max") EM (PMd/all_detectorsvsTd.py:135-173)."""
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d],
                        all_possibleSymbols, M, h_initial)
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode="hard", solve=solve)
    return _finish(res, verbose, itera)


def _x_from_zd(Z_d, Psi, n_tx, n_rx):
    """True data symbols from the genie regressors Z_d[t] = (psi_t (x) x_t)^T (x) I."""
    U = u_from_zp(Z_d, n_rx)                          # (T, P*n_tx)
    P = Psi.shape[0]
    U3 = U.reshape(U.shape[0], P, n_tx)
    p0 = np.argmax(np.abs(Psi), axis=0)               # a non-zero phase per symbol
    t = np.arange(U.shape[0])
    return U3[t, p0, :] / Psi[p0, t][:, None]


def em_llf(Y_d, Y_p, T_d, T_p, Z_p, Z_d, PsiTilde_td, all_possibleSymbols, M, varn, itera,
           h_initial, n_tx, mode="soft"):
    """Soft EM + per-iteration LLF (PMd/IterationsvsLLF.py:45-77).
    Returns (theta (K,1), logLikelihood (itera,1))."""
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d],
                        all_possibleSymbols, M, h_initial)
    if d["n_tx"] != n_tx:
        raise ValueError("n_tx does not match all_possibleSymbols")
    xd = _x_from_zd(Z_d[:T_d], np.asarray(PsiTilde_td)[:, :T_d], n_tx, d["n_rx"])[None]
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode=mode, x_d_true=xd)
    th = _finish(res, False, itera)
    return th, res["llf"][0].reshape(itera, 1)


def em_ml_llf(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
              h_initial, Z_d):
    """Hard-ML EM + LLF (PMd/ML_detecctor.py:51-86; the reference reads Z_d as a
    module global, here it is an explicit argument)."""
    n_tx = np.asarray(all_possibleSymbols).shape[1]
    return em_llf(Y_d, Y_p, T_d, T_p, Z_p, Z_d, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                  h_initial, n_tx, mode="hard")


def _pm(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, aps, M, varn, itera, h_initial, h, n_tx,
        partition_r, qamCons, mode, solve, verbose):
    cons = np.asarray(qamCons, dtype=complex).reshape(-1)
    if cons.size != int(M):
        raise ValueError("qamCons must hold the M constellation points")
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d], aps, M,
                        h_initial, n_tx=int(n_tx), cons=cons)
    if d["n_tx"] != int(n_tx):
        raise ValueError("n_tx does not match all_possibleSymbols")
    hh = None if h is None else np.asarray(h, dtype=complex).reshape(1, -1)
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], cons, varn, itera, d["theta0"],
                   mode=mode, h_true=hh, solve=solve, partition_r=int(partition_r))
    return _finish(res, verbose, itera)


def em_pm(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial, h,
          n_tx, partition_r, X_d, qamCons, verbose=False, solve="lstsq"):
    """Partitioned list-detector EM, every list member weight 1 (PMd/PM.py:47-116).

    The list of M**(p+1) candidates (p = int(partition_r / log2 M)) is built per
    symbol from the reference's off-by-one channel (PM.py:63) with greedy stream
    ordering and per-element slicing of the B partition; the candidate vector is
    the concatenation [x_A, x_B] used in natural stream order (PM.py:101-104).
    ``h`` drives the reference's oracle early stop (PM.py:110-112) when given;
    ``X_d`` is accepted for signature parity (the reference only reads its
    length).  ``all_possibleSymbols`` may be None (n_tx = 8 makes it 4.3e9 rows).
    The reference solves with lstsq (PM.py:108): solve='lstsq' (default) is its device
    counterpart, the minimum-norm solution with lstsq's singular-value cut."""
    return _pm(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
               h_initial, h, n_tx, partition_r, qamCons, "pm", solve, verbose)


def em_pm_soft(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, M, varn, itera, h_initial, h, n_tx,
               partition_r, X_d, qamCons, verbose=False, solve="chol"):
    """Partitioned list-detector EM with posterior list weights
    exp(-||y - H_t x||^2 / varn^2), normalised over the list (PMd/PM_beta.py:42-112;
    the same signature as PM_beta.em_pm, which takes no all_possibleSymbols)."""
    return _pm(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, None, M, varn, itera, h_initial, h, n_tx,
               partition_r, qamCons, "pm_soft", solve, verbose)


def _detector(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
              h_initial, h, mode, solve, verbose):
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d],
                        all_possibleSymbols, M, h_initial)
    hh = None if h is None else np.asarray(h, dtype=complex).reshape(1, -1)
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode=mode, h_true=hh, solve=solve)
    return _finish(res, verbose, itera)


def em_zf(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial, h,
          verbose=False, solve="chol"):
    """Zero-forcing detector EM (PMd/all_detectorsvsTd.py:98-133): per symbol
    z = pinv(H_off) y on the reference's off-by-one channel (:111), the flattened-argmin
    nearest_symbol_ecul decision (:49-52) as a weight-1 hypothesis, np.linalg.solve M-step,
    oracle early stop on h.  Where the reference's flat index runs past the hypothesis
    table (an IndexError there) the trial is flagged SBCE_STATUS_DETECTOR (last_status)."""
    return _detector(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                     h_initial, h, "zf", solve, verbose)


def em_mmse(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial,
            h, verbose=False, solve="chol"):
    """MMSE detector EM (PMd/all_detectorsvsTd.py:54-96): z = (H^H H + varn^2 I)^{-1} H^H y
    (:71), otherwise as em_zf.  (The reference's per-iteration LLF there reads a global
    Z_d and is never returned; it is not part of the result.)"""
    return _detector(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                     h_initial, h, "mmse", solve, verbose)


def _soft_linear(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, aps, M, varn, itera, h_initial, h, mode,
                 solve, verbose, ep_passes=None, prior_llr=None, labels=None):
    """_detector for the soft ZF / MMSE modes: all_possibleSymbols may also be the (M,) table
    itself (the M^n_tx hypothesis table is never enumerated and is out of reach at n_tx = 8);
    n_tx then follows from h_initial's length."""
    aps = np.asarray(aps)
    Psi = np.asarray(PsiTilde_td)[:, :T_d]
    if aps.ndim != 1:
        if mode != "ep":
            return _detector(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, aps, M, varn, itera, h_initial,
                             h, mode, solve, verbose)
        d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], Psi, aps, M, h_initial)
    else:
        n_tx = np.asarray(h_initial).size // (Psi.shape[0] * np.asarray(Y_d[0]).shape[0])
        d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], Psi, None, M, h_initial, n_tx=n_tx,
                            cons=aps[:int(M)])
    hh = None if h is None else np.asarray(h, dtype=complex).reshape(1, -1)
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode=mode, h_true=hh, solve=solve, ep_passes=ep_passes,
                   prior_llr=None if prior_llr is None else np.asarray(prior_llr)[None],
                   labels=labels)
    return _finish(res, verbose, itera)


def em_zf_soft(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
               h_initial, h, verbose=False, solve="chol"):
    """Soft zero-forcing EM for up to 8 streams (em_zf's argument list; n_rx >= n_tx): per symbol
    z = (H^H H)^{-1} H^H y on the clean effective channel, per-stream noise variance
    varn^2 (H^H H)^{-1}_aa, and the posterior moments of a Gaussian soft demapper per stream
    (include/sbce.h SBCE_ESTEP_ZF_SOFT) instead of em_zf's one-hot decision.  ``h`` drives the
    oracle early stop when given.  A symbol whose H^H H is singular carries the uniform
    posterior and flags the trial SBCE_STATUS_DETECTOR (last_status)."""
    return _soft_linear(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                        h_initial, h, "zf_soft", solve, verbose)


def em_mmse_soft(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                 h_initial, h, verbose=False, solve="chol"):
    """Soft MMSE EM for up to 8 streams (em_mmse's argument list): the unbiased LMMSE estimate
    with A = H^H H + (varn^2 / mean |cons|^2) I, otherwise as em_zf_soft (SBCE_ESTEP_MMSE_SOFT)."""
    return _soft_linear(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                        h_initial, h, "mmse_soft", solve, verbose)


def em_ep(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, h_initial, h,
          verbose=False, solve="chol", ep_passes=None, prior_llr=None, labels=None):
    """Expectation-propagation EM for up to 8 streams (em_mmse_soft's argument list): ``ep_passes``
    passes (None: 5; 1..16) of em_mmse_soft's solve per symbol, each with the demapper's
    per-stream means and variances of the pass before as the prior (include/sbce.h
    SBCE_ESTEP_EP); one pass is em_mmse_soft.  prior_llr (T_d,n_tx,log2 M): a-priori bit
    L-values of the data symbols with the labelling ``labels`` (None: Gray), as em_batch."""
    return _soft_linear(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
                        h_initial, h, "ep", solve, verbose, ep_passes, prior_llr, labels)


def em_ml_ser(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera,
              h_initial, verbose=False, solve="chol"):
    """Log-max EM of PMd/SER/log_max_SER.py:51-84: returns (theta (K,1), X_dest) with
    X_dest the list of (1, n_tx) argmax decisions of the last iteration (:77-78)."""
    d = _prepare_single(Y_d[:T_d], Y_p[:T_p], Z_p[:T_p], np.asarray(PsiTilde_td)[:, :T_d],
                        all_possibleSymbols, M, h_initial)
    res = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"], varn, itera, d["theta0"],
                   mode="hard", solve=solve, return_decisions=True)
    th = _finish(res, verbose, itera)
    return th, [x[None, :] for x in res["x_dest"][0]]


def em_superimposed(Y, T, Z, X_d, X_p, T_p, T_d, n_tx, PsiTilde_t, all_possibleSymbols, M, varn,
                    itera, N, verbose=False, solve="chol"):
    """Superimposed-pilot EM (Parallel/ParallelProtocol_Tp.py:63-86, same signature):
    T = max(T_d, T_p) symbols y_t carrying x_d,t + x_p,t (both zero-padded), soft
    posterior over x_j + x_p,t, no separate pilot block, theta_0 = 0.  Z is accepted for
    signature parity (the reference only passes it through)."""
    aps = np.asarray(all_possibleSymbols)
    n_tx = aps.shape[1]
    Psi = np.asarray(PsiTilde_t)[:, :T]
    n_rx = np.asarray(Y[0]).shape[0]
    Xp = np.zeros((T, n_tx), dtype=complex)
    xp = np.stack([np.asarray(x).reshape(-1) for x in X_p]) if len(X_p) else Xp[:0]
    Xp[:min(T, xp.shape[0])] = xp[:T]
    L = Psi.shape[0] * n_tx
    y = np.stack([np.asarray(v).reshape(-1) for v in Y[:T]])[None]
    res = em_batch(y, np.zeros((1, 0, n_rx), dtype=complex), Psi.T[None],
                   np.zeros((1, 0, L), dtype=complex), cons_from_aps(aps, int(M)), varn, itera,
                   np.zeros((1, L * n_rx), dtype=complex), mode="soft", solve=solve,
                   x_sup=Xp[None])
    return _finish(res, verbose, itera)


_GAUSS_CONS = np.array([1.0 + 0j, -1.0 + 0j])      # placeholder table: the Gaussian E-step has none


def gauss_expand_batch(theta, n_tx, n_rx, return_device=False):
    """The reference's n_rx x (N n_tx n_rx^2) channel matrix H_l (MIMO_Gaussian_proposed.py:
    77-85) from reduced Gaussian-EM estimates theta (B, N n_tx n_rx), on the device
    (sbce_gauss_expand)."""
    torch = _torch()
    lib = _lib.load()
    th = theta if isinstance(theta, torch.Tensor) else _dev(torch, theta, np.complex128)
    th = th.contiguous()
    B, K = th.shape
    P = K // (n_tx * n_rx)
    Q = P * n_tx * n_rx * n_rx
    dims = _lib.Dims(B, n_tx, n_rx, P, 0, 1, 2, 0, 1.0, 1.0)
    out = torch.empty((B, n_rx, Q), dtype=torch.complex128, device="cuda")
    _lib.check(lib.sbce_gauss_expand(dims, th.data_ptr(), out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "sbce_gauss_expand")
    if return_device:
        return out
    return out.cpu().numpy()


def gaussian_regressors(z_p, N, n_tx, n_rx):
    """u_p = psi_p (x) x_p from the reference's z_p = vec(kron(u_p^T, I_{n_rx})) =
    u_p (x) vec(I_{n_rx}) (received_proposed :126); raises if z_p has another structure."""
    L = N * n_tx
    e = np.eye(n_rx).flatten(order="F")
    if not len(z_p):
        return np.zeros((0, L), dtype=complex)
    Z = np.stack([np.asarray(z).reshape(-1) for z in z_p])
    if Z.shape[1] != L * n_rx * n_rx:
        raise ValueError(f"z_p has {Z.shape[1]} rows, expected N n_tx n_rx^2 = {L * n_rx * n_rx}")
    U = Z[:, ::n_rx * n_rx]                           # first vec(I) entry of each block (= 1)
    if not np.allclose(Z, np.einsum("tl,i->tli", U, e).reshape(Z.shape), rtol=1e-12, atol=0):
        raise ValueError("z_p is not kron(psi_p (x) x_p, vec(I_n_rx)) (received_proposed :126)")
    return U


def reduce_gaussian_channel(H, n_tx, n_rx):
    """Reduced channel theta[c n_rx + r] = H[r, c n_rx^2 : (c+1) n_rx^2] . vec(I): the only
    part of H the Gaussian E-step sees (H Sigma_t, Sigma_t = kron(., e e^H))."""
    H = np.asarray(H, dtype=complex)
    Lr = H.shape[1] // (n_rx * n_rx)
    Hr = np.einsum("rcjj->rc", H.reshape(n_rx, Lr, n_rx, n_rx))
    return Hr.T.reshape(-1)


last_gaussian_reduced = None


def EM_Gaussian_proposed(y_d, y_p, T_d, T_p, z_p, PsiTilde_td, varn, itera, H_initial, varx,
                         n_tx, verbose=False, solve="drop"):
    """Gaussian-prior EM (Proposed method/MIMO_Gaussian_proposed.py:56-89, same signature):
    x ~ CN(0, varx I) with the reference's prior covariance varx^2 kron(kron(psi psi^H, I),
    vec(I) vec(I)^H) (:33-45), itera + 1 iterations (``while j <= itera``), returns the
    n_rx x (N n_tx n_rx^2) matrix H_l.  The device runs the reduced form (include/sbce.h,
    SBCE_ESTEP_GAUSS / sbce_gauss_expand).  The reference's M-step inverse is the lstsq
    pseudo-inverse (:47-53), so the default solve is the pivot-dropping Cholesky ("drop"),
    identical to the plain inverse whenever the reduced G is well conditioned.  (At the
    script's own defaults the reference iteration diverges after one step, NMSE ~1e6 and
    growing; past that point neither its output nor this one is numerically meaningful.)"""
    global last_gaussian_reduced
    Psi = np.asarray(PsiTilde_td)[:, :T_d]
    N = Psi.shape[0]
    n_rx = np.asarray(y_d[0]).shape[0]
    U_p = gaussian_regressors(z_p[:T_p], N, n_tx, n_rx)
    yd = np.stack([np.asarray(v).reshape(-1) for v in y_d[:T_d]])[None]
    yp = (np.stack([np.asarray(v).reshape(-1) for v in y_p[:T_p]])[None] if T_p
          else np.zeros((1, 0, n_rx), dtype=complex))
    th0 = reduce_gaussian_channel(H_initial, n_tx, n_rx)[None]
    res = em_batch(yd, yp, Psi.T[None], U_p[None], _GAUSS_CONS, varn, int(itera) + 1, th0,
                   mode="gauss", solve=solve, varx=varx, return_device=True)
    torch = _torch()
    global last_status
    last_status = int(res["status"][0].item())
    last_gaussian_reduced = res["theta"][0].cpu().numpy()
    H = gauss_expand_batch(res["theta"], n_tx, n_rx)[0]
    if verbose:
        print(np.linalg.norm(H))
    torch.cuda.current_stream().synchronize()
    return H


def em_approx_batch(y_d, y_p, psi_d, psi_p, x_p, varn, updates, g0, return_device=False):
    """``updates`` updates of the semi-blind Gaussian-approximation EM (the comparator EM_approx
    of "Comparision/Comparision T_d vs NMSE.py":106-145) on a batch of independent trials: ONE
    sbce_approx_em call, which is one kernel launch (csrc/approx.hip).

    Layouts (complex128, batch-major, include/sbce.h): y_d (B,T_d,n_rx), y_p (B,T_p,n_rx),
    psi_d (B,T_d,N), psi_p (B,T_p,N), x_p (B,T_p), g0 (B,N,n_rx) = the initial value G_0
    (signal_model.initial_g_approx).  N <= 64, n_rx <= 8.  varn: one value or one per trial.
    Inputs may be numpy arrays or CUDA complex128 tensors.  Returns dict(g (B,N,n_rx), status
    (B,)): a trial whose normal matrix is singular (T_p + T_d < N) has SBCE_STATUS_SINGULAR set
    and keeps its last finite iterate."""
    torch = _torch()
    lib = _lib.load()
    Yd, Yp, Pd, Pp, Xp = (_cdev(torch, x) for x in (y_d, y_p, psi_d, psi_p, x_p))
    G = _cdev(torch, g0).clone()
    B, T_d, n_rx = Yd.shape
    T_p, N = Pp.shape[1], Pd.shape[2]
    if (Yp.shape != (B, T_p, n_rx) or Pd.shape != (B, T_d, N) or Pp.shape != (B, T_p, N)
            or Xp.reshape(B, -1).shape != (B, T_p) or G.shape != (B, N, n_rx)):
        raise ValueError("em_approx_batch: inconsistent shapes")
    varn0, Vt = _varn_arg(torch, varn, B)
    dims = _lib.ApproxDims(B, N, n_rx, T_p, T_d, 0, varn0)
    ws = _scratch(torch, lib.sbce_approx_workspace_bytes, "sbce_approx_workspace_bytes",
                  ctypes.byref(dims))
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    ptrs = _lib.ApproxPtrs(Yd.data_ptr(), Yp.data_ptr(), Pd.data_ptr(), Pp.data_ptr(),
                           Xp.data_ptr(), G.data_ptr(), Vt.data_ptr() if Vt is not None else None,
                           status.data_ptr(), ws.data_ptr(), ws.numel())
    _lib.check(lib.sbce_approx_em(dims, ptrs, int(updates),
                                  torch.cuda.current_stream().cuda_stream), "sbce_approx_em")
    return _result(torch, dict(g=G, status=status), return_device)


def EM_approx(PsiTilde_tp, PsiTilde_td, x_p, Y_p, Y_d, Iterations, varn, G=None, verbose=False):
    """Semi-blind Gaussian-approximation EM with the reference's signature and layouts
    ("Comparision/Comparision T_d vs NMSE.py":106-145): PsiTilde_tp N x L_p, PsiTilde_td N x L_d,
    x_p (L_p, 1), Y_p M x L_p, Y_d M x L_d.  G_0 is computed on the host (:107-108), the device
    runs Iterations + 1 updates (``while i <= Iterations``, :114) and the N x M estimate is
    returned.  ``G`` is accepted and unused, as in the reference, which only prints its norm."""
    from .signal_model import initial_g_approx
    global last_status
    Pp, Pd = np.asarray(PsiTilde_tp, dtype=complex), np.asarray(PsiTilde_td, dtype=complex)
    Yp, Yd = np.asarray(Y_p, dtype=complex), np.asarray(Y_d, dtype=complex)
    xp = np.asarray(x_p, dtype=complex).reshape(-1)
    G0 = initial_g_approx(Pp, xp, Yp)
    if verbose and G is not None:
        print("original G", np.linalg.norm(G))
    res = em_approx_batch(Yd.T[None], Yp.T[None], Pd.T[None], Pp.T[None], xp[None], varn,
                          int(Iterations) + 1, G0[None])
    last_status = int(res["status"][0])
    if verbose:
        print("G_Cap", np.linalg.norm(res["g"][0]))
    return res["g"][0]


_WANT = ("x_hat", "idx", "llr", "post")


def _detect_labels(cons_size, labels, need):
    """The labelling of a detect call: the given permutation, or the reference modem's Gray
    labelling when the table has a square-QAM size; None when none is needed or known."""
    from .qam import gray_labeling
    if labels is not None:
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        if lab.size != cons_size or not np.array_equal(np.sort(lab), np.arange(cons_size)):
            raise ValueError("labels must be a permutation of 0..M-1")
        return lab
    L = int(round(np.sqrt(cons_size)))
    if L * L == cons_size and not L & (L - 1):
        return gray_labeling(cons_size)
    if need:
        raise ValueError("this table has no default labelling: pass labels= for LLRs / bit errors")
    return None


def _detect_call(torch, Yd, Ps, Cs, Th, n_tx, sigma2, sigma2_t, lab, Xd, maxlog, want):
    """One sbce_detect on device tensors; returns the dict of device outputs."""
    lib = _lib.load()
    B, T_d, n_rx = Yd.shape
    P, M = Ps.shape[2], Cs.shape[0]
    if Ps.shape != (B, T_d, P) or Th.shape != (B, P * n_tx * n_rx):
        raise ValueError("detect: inconsistent shapes")
    lgM = max(int(M - 1).bit_length(), 1)
    bad = set(want) - set(_WANT)
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    out = {}
    if "x_hat" in want:
        out["x_hat"] = torch.empty((B, T_d, n_tx), dtype=torch.complex128, device="cuda")
    if "idx" in want:
        out["idx"] = torch.empty((B, T_d, n_tx), dtype=torch.int32, device="cuda")
    if "post" in want:
        out["post"] = torch.empty((B, T_d, n_tx, M), dtype=torch.float64, device="cuda")
    if "llr" in want:
        out["llr"] = torch.empty((B, T_d, n_tx, lgM), dtype=torch.float64, device="cuda")
    if Xd is not None and lab is not None:
        out["err"] = torch.empty((B, 2), dtype=torch.int32, device="cuda")

    def ptr(k):
        return out[k].data_ptr() if k in out else None

    dims = _lib.DetectDims(B, n_tx, n_rx, P, T_d, M, _lib.SBCE_DETECT_MAXLOG if maxlog else 0,
                           float(sigma2))
    nb = ctypes.c_size_t(0)
    _lib.check(lib.sbce_detect_workspace_bytes(ctypes.byref(dims), ctypes.byref(nb)),
               "sbce_detect_workspace_bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda") if nb.value else None
    ptrs = _lib.DetectPtrs(Yd.data_ptr(), Ps.data_ptr(), Cs.data_ptr(), Th.data_ptr(),
                           lab.data_ptr() if lab is not None else None,
                           sigma2_t.data_ptr() if sigma2_t is not None else None,
                           Xd.data_ptr() if Xd is not None else None,
                           ptr("x_hat"), ptr("idx"), ptr("post"), ptr("llr"), ptr("err"),
                           ws.data_ptr() if ws is not None else None, nb.value)
    _lib.check(lib.sbce_detect(dims, ptrs, torch.cuda.current_stream().cuda_stream), "sbce_detect")
    return out


def _sigma2_arg(torch, varn, B, noise):
    """(dims.sigma2, per-trial device tensor or None): the posterior denominator, varn**2 for the
    EM posterior (noise='em') or varn itself, the noise the data were drawn with (noise='true').
    varn: one value, a (B,) array, or the pair _varn_arg already made of one (EMEngine)."""
    if noise not in ("em", "true"):
        raise ValueError("noise must be 'em' or 'true'")
    v0, Vt = varn if isinstance(varn, tuple) else _varn_arg(torch, varn, B)
    if noise == "em":
        return v0 * v0, (Vt * Vt if Vt is not None else None)
    return v0, Vt


def detect_batch(y_d, psi_d, cons, theta, varn, n_tx, labels=None, x_d_true=None, noise="em",
                 maxlog=False, want=_WANT, return_device=False):
    """Decide the data symbols of a batch of trials from a channel estimate and say how good the
    decisions are: ONE sbce_detect call (one kernel launch, csrc/detect.hip).

    y_d (B,T_d,n_rx), psi_d (B,T_d,P), cons (M,) ANY table of M = 2..64 complex points, theta
    (B,K) any estimate in the E-step's layout (em_batch's theta, h_initial, the true h); numpy
    arrays or CUDA tensors.  varn: one value or (B,); noise='em' uses sigma^2 = varn**2 (the EM
    posterior), noise='true' sigma^2 = varn.  labels: an int permutation of 0..M-1 (bit i of
    symbol s = (labels[s] >> i) & 1); None means qam.gray_labeling for a square-QAM-sized table.
    Returns a dict with the outputs named in ``want``: x_hat (B,T_d,n_tx) and idx (int32 table
    indices) = the joint ML decision; post (B,T_d,n_tx,M) per-stream symbol posteriors; llr
    (B,T_d,n_tx,log2 M) L-values log(p0/p1), exact or (maxlog=True) max-log; with x_d_true
    also err (B,2) int32 = per-trial symbol and bit error counts."""
    torch = _torch()
    Yd, Ps, Cs, Th, Xd = (_cdev(torch, x) for x in (y_d, psi_d, cons, theta, x_d_true))
    lab = _detect_labels(Cs.shape[0], labels, "llr" in want or Xd is not None)
    lab_d = torch.from_numpy(lab).to("cuda") if lab is not None else None
    s2, s2t = _sigma2_arg(torch, varn, Yd.shape[0], noise)
    out = _detect_call(torch, Yd, Ps, Cs, Th, int(n_tx), s2, s2t, lab_d, Xd, maxlog, tuple(want))
    return _result(torch, out, return_device)


def detect(Y_d, PsiTilde_td, all_possibleSymbols, M, varn, theta, labels=None, X_d=None,
           noise="em", maxlog=False, want=_WANT):
    """detect_batch for one trial in the reference's list layouts (as em()): Y_d a list of
    (n_rx,1) observations, PsiTilde_td (N+1) x T_d, all_possibleSymbols the (M^n_tx, n_tx)
    hypothesis table, theta (K,1); X_d an optional list of true symbol vectors (error counts).
    Returns the dict of detect_batch without the batch axis."""
    aps = np.asarray(all_possibleSymbols)
    n_tx = aps.shape[1]
    cons = cons_from_aps(aps, int(M))
    T_d = len(Y_d)
    y = np.stack([np.asarray(v).reshape(-1) for v in Y_d])[None]
    psi = np.asarray(PsiTilde_td)[:, :T_d].T[None]
    xt = None if X_d is None else np.stack([np.asarray(x).reshape(-1) for x in X_d[:T_d]])[None]
    r = detect_batch(y, psi, cons, np.asarray(theta, dtype=complex).reshape(1, -1), varn, n_tx,
                     labels=labels, x_d_true=xt, noise=noise, maxlog=maxlog, want=want)
    return {k: v[0] for k, v in r.items()}


_WANT_LINEAR = ("x_soft", "nu", "x_hat", "idx", "llr", "post")
_WANT_LINEAR_ALL = _WANT_LINEAR + ("moments", "status")
_LINEAR_KINDS = {"mmse": _lib.SBCE_LINEAR_MMSE, "zf": _lib.SBCE_LINEAR_ZF,
                 "ep": _lib.SBCE_LINEAR_EP}


def _detect_linear_call(torch, Yd, Ps, Cs, Th, n_tx, kind, sigma2, sigma2_t, es, lab, Xd, maxlog,
                        want, ep_passes=None, la=None):
    """One sbce_detect_linear (la, the a-priori L-values on the device: sbce_detect_linear_prior)
    on device tensors; returns the dict of device outputs."""
    lib = _lib.load()
    B, T_d, n_rx = Yd.shape
    P, M = Ps.shape[2], Cs.shape[0]
    if Ps.shape != (B, T_d, P) or Th.shape != (B, P * n_tx * n_rx):
        raise ValueError("detect_linear: inconsistent shapes")
    if isinstance(kind, tuple):                        # ("ep", passes)
        if len(kind) != 2 or ep_passes is not None:
            raise ValueError("kind must be a name or ('ep', passes), the passes given once")
        kind, ep_passes = kind
    if kind not in _LINEAR_KINDS:
        raise ValueError("kind must be 'mmse', 'zf' or 'ep'")
    flags = (_lib.SBCE_DETECT_MAXLOG if maxlog else 0) | _lib.linear_ep_passes(
        _mode_word(kind, 0, ep_passes))
    lgM = max(int(M - 1).bit_length(), 1)
    bad = set(want) - set(_WANT_LINEAR_ALL)
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    c128, f64, i32 = torch.complex128, torch.float64, torch.int32
    shapes = {"x_soft": ((B, T_d, n_tx), c128), "nu": ((B, T_d, n_tx), f64),
              "x_hat": ((B, T_d, n_tx), c128), "idx": ((B, T_d, n_tx), i32),
              "post": ((B, T_d, n_tx, M), f64), "llr": ((B, T_d, n_tx, lgM), f64),
              "moments": ((B, T_d, n_tx + n_tx * n_tx), c128), "status": ((B,), i32)}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device="cuda")
           for k in _WANT_LINEAR_ALL if k in want}
    if Xd is not None and lab is not None:
        out["err"] = torch.empty((B, 2), dtype=i32, device="cuda")

    def ptr(k):
        return out[k].data_ptr() if k in out else None

    dims = _lib.LinearDims(B, n_tx, n_rx, P, T_d, M, _LINEAR_KINDS[kind], flags, float(sigma2),
                           float(es))
    nb = ctypes.c_size_t(0)
    _lib.check(lib.sbce_detect_linear_workspace_bytes(ctypes.byref(dims), ctypes.byref(nb)),
               "sbce_detect_linear_workspace_bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda") if nb.value else None
    ptrs = _lib.LinearPtrs(Yd.data_ptr(), Ps.data_ptr(), Cs.data_ptr(), Th.data_ptr(),
                           lab.data_ptr() if lab is not None else None,
                           sigma2_t.data_ptr() if sigma2_t is not None else None,
                           Xd.data_ptr() if Xd is not None else None,
                           ptr("x_soft"), ptr("nu"), ptr("x_hat"), ptr("idx"), ptr("post"),
                           ptr("llr"), ptr("err"), ptr("moments"), ptr("status"),
                           ws.data_ptr() if ws is not None else None, nb.value)
    stream = torch.cuda.current_stream().cuda_stream
    if la is None:
        _lib.check(lib.sbce_detect_linear(dims, ptrs, stream), "sbce_detect_linear")
    else:
        _lib.check(lib.sbce_detect_linear_prior(dims, ptrs, la.data_ptr(), stream),
                   "sbce_detect_linear_prior")
    return out


def _linear_es(torch, cons, es):
    """The MMSE prior's symbol energy: the given value, or mean |cons|^2 of the table (taken on
    the host from an array; a device tensor costs one synchronising copy)."""
    if es is not None:
        return float(es)
    c = cons.cpu().numpy() if isinstance(cons, torch.Tensor) else np.asarray(cons)
    return float(np.mean(np.abs(c) ** 2))


def detect_linear_batch(y_d, psi_d, cons, theta, varn, n_tx, kind="mmse", es=None, labels=None,
                        x_d_true=None, noise="em", maxlog=False, want=_WANT_LINEAR,
                        return_device=False):
    """Linear soft detection of a batch of trials from a channel estimate, for n_tx = 1..8: ONE
    sbce_detect_linear call (the detection kernel of csrc/detect_linear.hip, preceded by a small
    zeroing kernel when err or status is produced).

    Arguments as detect_batch.  kind: 'mmse' (LMMSE equaliser with the prior energy ``es``; None
    means mean |cons|^2, 1 gives the reference's filter of all_detectorsvsTd.py:71) or 'zf' (needs
    n_rx >= n_tx) or 'ep' (expectation propagation, SBCE_LINEAR_EP: 5 passes of the 'mmse' solve,
    or ('ep', p) for p = 1..16 passes; x_soft and nu are then the extrinsic estimate and variance
    of the last pass).  Returns a dict with the outputs named in ``want``: x_soft (B,T_d,n_tx) the
    unbiased per-stream estimate and nu its effective noise variance; x_hat / idx the per-stream
    nearest table point; post (B,T_d,n_tx,M) and llr (B,T_d,n_tx,log2 M) of the Gaussian demapper
    (exact or, maxlog=True, max-log); moments (B,T_d,n_tx+n_tx^2) in estep_batch's layout; status
    (B,) int32, SBCE_STATUS_NONHPD where a symbol's matrix had a failed pivot (that symbol:
    x_soft = 0, nu = inf, post = 1/M, llr = 0); with x_d_true also err (B,2) int32.
    With a-priori bit L-values: detect_linear_prior_batch."""
    return _detect_linear_batch(y_d, psi_d, cons, theta, varn, n_tx, kind, es, labels, x_d_true,
                                noise, maxlog, want, return_device, None)


def detect_linear_prior_batch(y_d, psi_d, cons, theta, varn, n_tx, prior_llr, kind="ep", es=None,
                              labels=None, x_d_true=None, noise="em", maxlog=False,
                              want=_WANT_LINEAR, return_device=False):
    """detect_linear_batch with a-priori bit L-values (sbce_detect_linear_prior, soft-input EP; a
    function of its own because detect_linear_batch's argument list is fixed): prior_llr
    (B,T_d,n_tx,log2 M) = log(P(bit = 0) / P(bit = 1)) under ``labels`` (None: Gray), NaN read as
    0 and +-inf as a known bit; kind 'ep' or ('ep', p) only -- one pass is the soft-cancellation
    MMSE turbo detector.  x_soft, nu and llr are then extrinsic (stream a's own prior is not in
    them), post, moments and the decisions a-posteriori; a failed symbol has post = the
    a-priori pmf and llr = 0.  prior_llr=None is detect_linear_batch."""
    return _detect_linear_batch(y_d, psi_d, cons, theta, varn, n_tx, kind, es, labels, x_d_true,
                                noise, maxlog, want, return_device, prior_llr)


def _detect_linear_batch(y_d, psi_d, cons, theta, varn, n_tx, kind, es, labels, x_d_true, noise,
                         maxlog, want, return_device, prior_llr):
    torch = _torch()
    es = _linear_es(torch, cons, es)                   # from the caller's table, before the upload
    Yd, Ps, Cs, Th, Xd = (_cdev(torch, x) for x in (y_d, psi_d, cons, theta, x_d_true))
    lab = _detect_labels(Cs.shape[0], labels,
                         "llr" in want or Xd is not None or prior_llr is not None)
    lab_d = torch.from_numpy(lab).to("cuda") if lab is not None else None
    s2, s2t = _sigma2_arg(torch, varn, Yd.shape[0], noise)
    la, _ = _prior_arg(torch, prior_llr, lab_d, Yd.shape[0], Yd.shape[1], int(n_tx), Cs.shape[0],
                       kind[0] if isinstance(kind, tuple) else kind)
    out = _detect_linear_call(torch, Yd, Ps, Cs, Th, int(n_tx), kind, s2, s2t, es, lab_d, Xd,
                              maxlog, tuple(want), la=la)
    return _result(torch, out, return_device)


def detect_linear(Y_d, PsiTilde_td, all_possibleSymbols, M, varn, theta, kind="mmse", es=None,
                  labels=None, X_d=None, noise="em", maxlog=False, want=_WANT_LINEAR,
                  ep_passes=None, prior_llr=None):
    """detect_linear_batch for one trial in the reference's list layouts (as detect()).
    all_possibleSymbols may also be the (M,) table itself (the M^n_tx hypothesis table is never
    enumerated here and is out of reach at n_tx = 8); n_tx then follows from theta's length.
    ep_passes: the pass count of kind 'ep' (None: 5), as kind=('ep', ep_passes).
    prior_llr (T_d,n_tx,log2 M): a-priori bit L-values, as detect_linear_prior_batch.
    Returns the dict of detect_linear_batch without the batch axis."""
    aps = np.asarray(all_possibleSymbols)
    T_d = len(Y_d)
    y = np.stack([np.asarray(v).reshape(-1) for v in Y_d])[None]
    psi = np.asarray(PsiTilde_td)[:, :T_d].T[None]
    if aps.ndim == 1:
        cons = aps[:int(M)].astype(complex)
        n_tx = np.asarray(theta).size // (psi.shape[2] * y.shape[2])
    else:
        n_tx = aps.shape[1]
        cons = cons_from_aps(aps, int(M))
    xt = None if X_d is None else np.stack([np.asarray(x).reshape(-1) for x in X_d[:T_d]])[None]
    r = detect_linear_prior_batch(y, psi, cons, np.asarray(theta, dtype=complex).reshape(1, -1),
                                  varn, n_tx,
                                  None if prior_llr is None else np.asarray(prior_llr)[None],
                                  kind=kind if ep_passes is None else (kind, ep_passes), es=es,
                                  labels=labels, x_d_true=xt, noise=noise, maxlog=maxlog, want=want)
    return {k: v[0] for k, v in r.items()}


def ser_batch(x_dest, x_d_true):
    """Per-trial SER on the device (sbce_ser): (ser_reference, ser_elementwise), the first
    being the expression of PMd/SER/log_max_SER.py:162."""
    torch = _torch()
    lib = _lib.load()
    xd = x_dest if isinstance(x_dest, torch.Tensor) else _dev(torch, x_dest, np.complex128)
    xt = x_d_true if isinstance(x_d_true, torch.Tensor) else _dev(torch, x_d_true, np.complex128)
    B, T_d, n_tx = xd.shape
    dims = _lib.Dims(B, n_tx, 1, 1, 0, T_d, 2, 0, 1.0)
    out = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
    _lib.check(lib.sbce_ser(dims, xd.contiguous().data_ptr(), xt.contiguous().data_ptr(),
                            out.data_ptr(), torch.cuda.current_stream().cuda_stream), "sbce_ser")
    out = out.cpu().numpy()
    return out[:, 0], out[:, 1]


def em_zero_init(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera):
    """Root-level em() (Proposed_method_NMSEvsTp.py:43-69): theta_0 = 0."""
    return em(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn, itera, None)


# ------------------------------------------------------------------ diagnostic stages
def estep_batch(y_d, psi_d, cons, theta, varn, n_tx, mode="soft", partition_r=0, varx=1.0,
                workspace=True, return_status=False, ep_passes=None, prior_llr=None, labels=None):
    """One device E-step (sbce_estep): returns m (B,T_d,n_tx), S (B,T_d,n_tx,n_tx) and, with
    return_status, the (B,) status words (SBCE_STATUS_DETECTOR: a ZF / MMSE decision past the
    hypothesis table, or a failed pivot of a symbol in "mmse_soft" / "zf_soft" / "ep").  mode: any of
    em_batch's ("ep" with ``ep_passes``).  varn may be one value or one per trial ((B,), as em_batch takes it).
    workspace=False passes no workspace (the exact sweep then prepares each symbol in
    its own kernel instead of the separate preparation pass).  prior_llr / labels (mode "ep"):
    a-priori bit L-values as em_batch (sbce_estep_prior)."""
    torch = _torch()
    lib = _lib.load()
    B, T_d, n_rx = np.shape(y_d)
    P = np.shape(psi_d)[2]
    y_p = np.zeros((B, 0, n_rx), dtype=complex)
    u_p = np.zeros((B, 0, P * n_tx), dtype=complex)
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta, varn,
                 _mode_word(mode, partition_r, ep_passes), varx,
                 check="theta" if np.ndim(varn) else None, workspace=workspace)
    mom = torch.zeros((B, T_d, n_tx + n_tx * n_tx), dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    pr = _Prior(*_prior_arg(torch, prior_llr, labels, B, T_d, n_tx, st.M, mode))
    if pr.opts is None:
        _lib.check(lib.sbce_estep(st.dims, st.ptrs(), _MODES[mode], mom.data_ptr(), stream),
                   "sbce_estep")
    else:
        _lib.check(lib.sbce_estep_prior(st.dims, st.ptrs(), _MODES[mode], pr.ref(), mom.data_ptr(),
                                        stream), "sbce_estep_prior")
    torch.cuda.current_stream().synchronize()
    mom = mom.cpu().numpy()
    out = mom[..., :n_tx], mom[..., n_tx:].reshape(B, T_d, n_tx, n_tx)
    return (*out, st.status.cpu().numpy()) if return_status else out


def mstep_batch(y_d, y_p, psi_d, u_p, cons, m, S, varn, solve="chol", return_tol=False,
                ws_fill=None):
    """One device M-step (sbce_mstep) from given moments: returns theta (B,K),
    R (B,L,L), rhs (B,L,n_rx), status (B,) [, tol (B,): the min-norm pivot threshold
    32 eps K lambda_max(R) (sbce_debug_minnorm_tol), return_tol=True with solve='lstsq'].
    ws_fill: a byte value the workspace is filled with first (tests: results must not
    depend on what a workspace held)."""
    torch = _torch()
    lib = _lib.load()
    B, T_d, n_rx = np.shape(y_d)
    L = np.shape(u_p)[2]
    n_tx = np.shape(m)[2]
    theta = np.zeros((B, L * n_rx), dtype=complex)
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, theta, varn)
    dims, ptrs = st.dims, st.ptrs()
    if ws_fill is not None:
        st.ws.fill_(int(ws_fill))
    mom = np.concatenate([np.asarray(m).reshape(B, T_d, n_tx),
                          np.asarray(S).reshape(B, T_d, n_tx * n_tx)], axis=2)
    Mo = _dev(torch, mom, np.complex128)
    R = torch.zeros((B, L, L), dtype=torch.complex128, device="cuda")
    rhs = torch.zeros((B, L, n_rx), dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sbce_mstep(dims, ptrs, Mo.data_ptr(), _SOLVES[solve], R.data_ptr(),
                              rhs.data_ptr(), stream), "sbce_mstep")
    tol = None
    if return_tol:
        tol = np.zeros(B)
        fn = lib.sbce_debug_minnorm_tol
        fn.restype = ctypes.c_int
        torch.cuda.current_stream().synchronize()
        _lib.check(fn(ctypes.byref(dims), ctypes.byref(ptrs), tol.ctypes.data_as(ctypes.c_void_p),
                      ctypes.c_void_p(stream)), "sbce_debug_minnorm_tol")
    torch.cuda.current_stream().synchronize()
    th = st.theta.cpu().numpy()
    # the device keeps only R's lower triangle (its strict upper part is factorisation
    # workspace): return the Hermitian completion
    R = np.tril(R.cpu().numpy())
    R = R + np.conj(np.swapaxes(np.tril(R, -1), 1, 2))
    out = (th, R, rhs.cpu().numpy(), st.status.cpu().numpy())
    return out + (tol,) if return_tol else out


def nmse_batch(theta, h):
    """Per-trial NMSE on the device (sbce_nmse), PMd/Proposed_method_NMSEvsTp.py:172."""
    torch = _torch()
    lib = _lib.load()
    th = theta if isinstance(theta, torch.Tensor) else _dev(torch, theta, np.complex128)
    hh = h if isinstance(h, torch.Tensor) else _dev(torch, h, np.complex128)
    B, K = th.shape
    dims = _lib.Dims(B, 1, 1, K, 0, 1, 2, 0, 1.0)   # only batch and K = n_psi*n_tx*n_rx matter
    out = torch.zeros(B, dtype=torch.float64, device="cuda")
    _lib.check(lib.sbce_nmse(dims, th.data_ptr(), hh.data_ptr(), out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream), "sbce_nmse")
    return out


# ------------------------------------------------------------------ Cramer-Rao bounds
_WANT_CRB = ("tr_inv", "mse", "diag_inv")


def genie_moments(x_d):
    """Moments of known data symbols x_d (..., n_tx): m = x, S = x x^H -- the E-step's output when
    every posterior is a point mass, and the input of the all-data-known bound (crb_batch)."""
    x = np.asarray(x_d, dtype=complex)
    return x, x[..., :, None] * np.conj(x[..., None, :])


def _crb_call(torch, lib, dims, ptrs, mom, sigma2, sigma2_t, have_h, want, scratch_fill=None):
    """One sbce_crb on staged buffers (current stream): dict of device tensors tr_inv (B,), and by
    ``want`` mse (B,), diag_inv (B,L); bound (B,) when ptrs carries h_true."""
    bad = set(want) - set(_WANT_CRB) - {"bound"}
    if bad:
        raise ValueError(f"crb: unknown output {sorted(bad)}")
    B, L = dims.batch, dims.n_psi * dims.n_tx
    scratch = _scratch(torch, lib.sbce_crb_workspace_bytes, "sbce_crb_workspace_bytes",
                       ctypes.byref(dims))
    if scratch_fill is not None:
        scratch.fill_(int(scratch_fill))
    out = dict(tr_inv=torch.zeros(B, dtype=torch.float64, device="cuda"))
    if "mse" in want or have_h:
        out["mse"] = torch.zeros(B, dtype=torch.float64, device="cuda")
    if "diag_inv" in want:
        out["diag_inv"] = torch.zeros((B, L), dtype=torch.float64, device="cuda")
    if have_h:
        out["bound"] = torch.zeros(B, dtype=torch.float64, device="cuda")
    ptr = lambda k: out[k].data_ptr() if k in out else None
    opts = _lib.CrbOpts(float(sigma2), sigma2_t.data_ptr() if sigma2_t is not None else None,
                        ptr("tr_inv"), ptr("diag_inv"), ptr("mse"), ptr("bound"),
                        scratch.data_ptr(), scratch.numel(), 0)
    _lib.check(lib.sbce_crb(dims, ptrs, mom.data_ptr(), opts,
                            torch.cuda.current_stream().cuda_stream), "sbce_crb")
    return out                         # the scratch is used in stream order: it may be freed now


def crb_batch(y_d, y_p, psi_d, u_p, cons, n_tx, sigma2, kind="genie", m=None, S=None,
              x_d_true=None, h_true=None, want=_WANT_CRB, ws_fill=None):
    """Cramer-Rao bound of the cascaded-channel estimate per trial (sbce_crb, csrc/crb.hip): with
    R = sum_p u_p u_p^H + sum_t (psi_t psi_t^H) (x) S_t the least-squares estimate with known
    regressors has E||theta_hat - theta||^2 = n_rx sigma2 tr(R^-1), coefficient (l, r) the variance
    sigma2 (R^-1)_ll.  kind selects the moments fed to the build:
      "pilot"    S_t = 0: the pilot-only bound (+inf where the pilots alone do not identify the
                 channel -- always so for signal_model's dft_n pilots -- or T_p < L)
      "genie"    m_t = x_t, S_t = x_t x_t^H from x_d_true (B,T_d,n_tx): all data known, the floor
                 of every semi-blind curve; finite only when T_p + T_d >= L
      "moments"  m (B,T_d,n_tx), S (B,T_d,n_tx,n_tx) as given (estep_batch's outputs): the
                 complete-data error variance of the estimate made from them -- optimistic, it
                 ignores the information lost to symbol uncertainty.
    sigma2: the noise variance the data carry (the signal model's varn, NOT the posterior's
    varn**2), one value or (B,).  y_d / y_p may be None (R does not depend on them; zeros are
    staged).  h_true (B,K): also ``bound`` = mse / ||h||^2, the bound on the NMSE.
    A trial with a Cholesky pivot not above 1e-14 max diag R is unidentifiable: every output +inf and
    SBCE_STATUS_NONHPD in ``status``.  ws_fill: a byte the workspace and scratch are filled with first (tests).
    Returns dict(tr_inv (B,), status (B,) [, mse (B,), diag_inv (B,L), bound (B,)]) as numpy arrays."""
    if kind not in ("genie", "pilot", "moments"):
        raise ValueError(f"crb_batch: unknown kind {kind!r}")
    n_tx = int(n_tx)
    B, T_d, P = np.shape(psi_d)
    L = P * n_tx
    if np.shape(u_p)[2] != L:
        raise ValueError("u_p width must be P*n_tx")
    if kind == "genie":
        if x_d_true is None:
            raise ValueError("crb_batch: kind 'genie' needs x_d_true")
        m, S = genie_moments(np.asarray(x_d_true).reshape(B, T_d, n_tx))
    elif kind == "pilot":
        m, S = np.zeros((B, T_d, n_tx), dtype=complex), np.zeros((B, T_d, n_tx, n_tx), dtype=complex)
    elif m is None or S is None:
        raise ValueError("crb_batch: kind 'moments' needs m and S")
    if np.shape(m) != (B, T_d, n_tx) or np.shape(S) != (B, T_d, n_tx, n_tx):
        raise ValueError("crb_batch: m must be (B,T_d,n_tx) and S (B,T_d,n_tx,n_tx)")
    if y_d is not None:
        n_rx = np.shape(y_d)[2]
    elif y_p is not None:
        n_rx = np.shape(y_p)[2]
    else:
        n_rx = np.shape(h_true)[1] // L if h_true is not None else 1
    T_p = np.shape(u_p)[1]
    if y_d is None:
        y_d = np.zeros((B, T_d, n_rx), dtype=complex)
    if y_p is None:
        y_p = np.zeros((B, T_p, n_rx), dtype=complex)
    torch = _torch()
    lib = _lib.load()
    s2, s2t = _varn_arg(torch, sigma2, B)
    st = _Staged(torch, y_d, y_p, psi_d, u_p, cons, np.zeros((B, L * n_rx), dtype=complex), 1.0,
                 solve=_lib.SBCE_SOLVE_CHOL)
    if ws_fill is not None:
        st.ws.fill_(int(ws_fill))
    mom = _dev(torch, np.concatenate([np.asarray(m).reshape(B, T_d, n_tx),
                                      np.asarray(S).reshape(B, T_d, n_tx * n_tx)], axis=2),
               np.complex128)
    Ht = _cdev(torch, h_true)
    out = _crb_call(torch, lib, st.dims, st.ptrs(h_true=Ht), mom, s2, s2t, Ht is not None,
                    tuple(want), ws_fill)
    out["status"] = st.status
    torch.cuda.current_stream().synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()
            if k in want or k in ("tr_inv", "status", "bound")}


# ------------------------------------------------------------------ decoder and the turbo loop
_WANT_SISO = ("le_c", "lapp_u", "u_hat")


def _f64dev(torch, x):
    """A float64 input as a contiguous CUDA tensor (None stays None)."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda", dtype=torch.float64).contiguous()
    return _dev(torch, x, np.float64)


def _i32dev(torch, x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda", dtype=torch.int32).contiguous()
    return _dev(torch, x, np.int32)


def siso_decode_batch(lc, code, prior_u=None, perm=None, u_true=None, maxlog=False,
                      want=_WANT_SISO, return_device=False, ws_fill=None):
    """Soft-in / soft-out decoding of a batch of codewords: ONE sbce_siso_decode call (the BCJR
    kernel of csrc/siso.hip, preceded by a small zeroing kernel when err is produced).

    lc (B, n_steps*n): L-values log(P(bit = 0) / P(bit = 1)) of the received coded bits, e.g. a
    detector's flattened ``llr``; code: a codec.ConvCode; prior_u (B, n_info): a-priori L-values
    of the information bits; perm (n_steps*n,) int32: coded bit k sits at position perm[k] of lc
    and of le_c (codec.random_interleaver; a bijection, not checked on the device); u_true
    (B, n_info) 0/1: also err (B,) int32, the bit errors of u_hat; maxlog: max-log-MAP.  NaN is
    read as 0 and every value is clamped to +-64.  Inputs may be numpy arrays or CUDA tensors
    (used in place).  ws_fill: a byte the workspace is filled with first (tests).
    Returns a dict with the outputs named in ``want``: le_c (B, n_steps*n) the EXTRINSIC L-values
    of the coded bits (what the detector takes as prior_llr), lapp_u (B, n_info) the a-posteriori
    L-values and u_hat (B, n_info) int32 the decisions."""
    torch = _torch()
    lib = _lib.load()
    bad = set(want) - set(_WANT_SISO)
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    Lc, La, Pm, Ut = (_f64dev(torch, lc), _f64dev(torch, prior_u), _i32dev(torch, perm),
                      _i32dev(torch, u_true))
    if Lc.dim() != 2:
        raise ValueError("lc must be (B, n_steps*n)")
    B, nc = Lc.shape
    n_info = code.n_info_for(nc)
    if La is not None and tuple(La.shape) != (B, n_info):
        raise ValueError(f"prior_u shape {tuple(La.shape)} != {(B, n_info)}")
    if Ut is not None and tuple(Ut.shape) != (B, n_info):
        raise ValueError(f"u_true shape {tuple(Ut.shape)} != {(B, n_info)}")
    if Pm is not None and tuple(Pm.shape) != (nc,):
        raise ValueError(f"perm shape {tuple(Pm.shape)} != {(nc,)}")
    gens = tuple(code.generators) + (0,) * (3 - code.n)
    flags = ((_lib.SBCE_DETECT_MAXLOG if maxlog else 0) |
             (_lib.SBCE_SISO_TERMINATED if code.terminated else 0))
    dims = _lib.SisoDims(B, n_info, code.K, code.n, (ctypes.c_int32 * 3)(*gens), flags)
    f64, i32 = torch.float64, torch.int32
    shapes = {"le_c": ((B, nc), f64), "lapp_u": ((B, n_info), f64), "u_hat": ((B, n_info), i32)}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device="cuda")
           for k in _WANT_SISO if k in want}
    if Ut is not None:
        out["err"] = torch.empty(B, dtype=i32, device="cuda")
    ws = _scratch(torch, lib.sbce_siso_workspace_bytes, "sbce_siso_workspace_bytes",
                  ctypes.byref(dims))
    if ws_fill is not None:
        ws.fill_(int(ws_fill))

    def ptr(t):
        return t.data_ptr() if t is not None else None

    ptrs = _lib.SisoPtrs(Lc.data_ptr(), ptr(La), ptr(Pm), ptr(Ut), ptr(out.get("lapp_u")),
                         ptr(out.get("u_hat")), ptr(out.get("le_c")), ptr(out.get("err")),
                         ws.data_ptr(), ws.numel())
    _lib.check(lib.sbce_siso_decode(dims, ptrs, torch.cuda.current_stream().cuda_stream),
               "sbce_siso_decode")
    return _result(torch, out, return_device)      # the workspace is used in stream order


def turbo_em_batch(y_d, y_p, psi_d, u_p, cons, varn, theta0, n_tx, code, perm, outer=4, itera=3,
                   ep_passes=None, labels=None, noise="true", u_true=None, h_true=None):
    """The code-aided (turbo) loop: channel estimation, detection and decoding exchanging soft
    information.  With la^0 = no prior and theta_0 = theta0, for k = 1..outer:
      theta_k = em_batch(mode="ep", prior_llr=la^{k-1}, theta0=theta_{k-1}), ``itera`` iterations
      llr     = detect_linear_prior_batch(theta_k, la^{k-1}): the detector's extrinsic L-values
      la^k    = siso_decode_batch(llr flattened per trial, perm)'s le_c, reshaped to
                (B, T_d, n_tx, log2 M); u_hat the decoder's decisions
    One codeword spans the T_d n_tx log2 M bits of a trial: bit i of stream a of symbol t is
    position (t n_tx + a) log2 M + i, and coded bit k travels at position perm[k].
    varn: the noise variance the data carry.  noise="true": the EM is given sqrt(varn), whose
    square its posterior divides by, and the detector varn (exit_chart.py's convention);
    noise="em": both are given varn as the reference's EM parameter.  The L-values stay on the
    device between the three calls.
    Returns a list of ``outer`` dicts of numpy arrays: theta (B,K), u_hat (B,n_info) and, with
    u_true (B,n_info), bit_errors (B,); with h_true (B,K), nmse (B,)."""
    torch = _torch()
    if noise not in ("em", "true"):
        raise ValueError("noise must be 'em' or 'true'")
    n_tx = int(n_tx)
    Yd, Yp, Ps, Up, Cs, theta = (_cdev(torch, x) for x in (y_d, y_p, psi_d, u_p, cons, theta0))
    Ht = _cdev(torch, h_true)
    B, T_d = Yd.shape[0], Yd.shape[1]
    M = Cs.shape[0]
    lgM = max(int(M - 1).bit_length(), 1)
    code.n_info_for(T_d * n_tx * lgM)                  # raises when a trial is no codeword
    lab_np = _detect_labels(M, labels, True)
    es = _linear_es(torch, cons, None)
    Pm, Ut = _i32dev(torch, perm), _i32dev(torch, u_true)
    v0, Vt = _varn_arg(torch, varn, B)
    varn_em = varn if noise == "em" else (float(np.sqrt(v0)) if Vt is None else torch.sqrt(Vt))
    kind = "ep" if ep_passes is None else ("ep", int(ep_passes))
    la, out = None, []
    for _ in range(int(outer)):
        em = em_batch(Yd, Yp, Ps, Up, Cs, varn_em, int(itera), theta, mode="ep",
                      ep_passes=ep_passes, prior_llr=la, labels=lab_np, return_device=True)
        theta = em["theta"]
        det = detect_linear_prior_batch(Yd, Ps, Cs, theta, varn, n_tx, la, kind=kind, es=es,
                                        labels=lab_np, noise=noise, want=("llr",),
                                        return_device=True)
        dec = siso_decode_batch(det["llr"].reshape(B, -1), code, perm=Pm, u_true=Ut,
                                want=("le_c", "u_hat"), return_device=True)
        la = dec["le_c"].reshape(B, T_d, n_tx, lgM)
        res = dict(theta=theta, u_hat=dec["u_hat"])
        if Ut is not None:
            res["bit_errors"] = dec["err"]
        if Ht is not None:
            res["nmse"] = nmse_batch(theta, Ht)
        out.append(res)
    torch.cuda.current_stream().synchronize()
    return [{k: v.cpu().numpy() for k, v in r.items()} for r in out]


class EMEngine:
    """Pre-allocated device state for repeated batched EM runs (benchmark / sweeps).

    All buffers (observations, phases, pilot regressors, theta, workspace) stay
    resident in HBM; ``run()`` resets theta from theta0 with a device copy and
    issues ONE sbce_em call on the current stream.  Nothing is allocated or
    synchronised inside ``run()``.

    ``streams = K > 1``: ``run()`` issues the batch as K contiguous sub-batches, each on its own HIP
    stream (forked from and joined back into the current stream), through ONE sbce_em_multi call:
    where the fixed-point rule is armed the launch sequence of a sub-batch ends once all its
    trials are frozen, so run() may wait for the device (include/sbce.h); ``iters_issued`` holds
    the iterations the last run() enqueued per sub-batch.
    Trials are independent and every kernel treats them independently, so theta is bitwise
    the same; the sub-batches' kernels overlap -- the latency-bound launches of one (the
    Cholesky panel factors, the enumeration tail) run beside the MFMA-bound ones of another.
    Each sub-batch has its own workspace (its work lists and counters are per call); the
    inputs, theta and status are views of the whole-batch tensors.  ``estep()``, ``mstep()``
    and ``mstep_phase()`` (kernel timing) stay whole-batch launches.
    """

    def __init__(self, batch, varn, mode="soft", solve="chol", x_d_true=None, h_true=None,
                 partition_r=0, varx=1.0, x_sup=None, streams=1, early_stop=False, ep_passes=None,
                 prior_llr=None, labels=None):
        """ep_passes: the pass count of mode "ep" (None: 5).  prior_llr (B,T_d,n_tx,log2 M) with
        ``labels`` (None: Gray): a-priori bit L-values of the data symbols (mode "ep", one stream);
        run(), capture(), estep() and detect_linear(kind="ep") then use them.  early_stop=True: the reference's oracle early stop on the true channel (PM.py:110-112,
        all_detectorsvsTd.py's five EMs) with h_true (or batch["h"]); ``iters_done`` then holds
        the iterations each trial of the last run() performed."""
        torch = _torch()
        self.torch = torch
        partition_r = _mode_word(mode, partition_r, ep_passes)
        # varn: one noise variance, or one per trial (the SNR axis of a sweep batched into one
        # call).  The engine owns the workspace (below): the staged problem gets none of its own.
        st = _Staged(torch, batch["y_d"], batch["y_p"], batch["psi_d"], batch["u_p"], batch["cons"],
                     batch["theta0"], varn, partition_r, varx, check="theta0", clone=True,
                     workspace=False)
        for k in ("y_d", "y_p", "psi_d", "u_p", "cons", "theta0", "theta", "n_tx", "n_rx", "B",
                  "T_d", "T_p", "P", "M", "varn", "varn_t", "dims", "status", "iters_done"):
            setattr(self, k, getattr(st, k))
        B, T_d, n_rx, T_p, P = st.B, st.T_d, st.n_rx, st.T_p, st.P
        self.h = _cdev(torch, h_true if h_true is not None else batch.get("h"))
        if mode == "gauss" and not varx > 0:
            raise ValueError("mode 'gauss' needs a prior variance varx > 0")
        if x_sup is not None and mode not in ("soft", "hard"):
            raise ValueError("superimposed pilots (x_sup) need the soft or hard E-step")
        self.mode, self.solve = _MODES[mode], _SOLVES[solve]
        # ONE device buffer: the whole-batch workspace (estep / mstep / mstep_phase) and, when the
        # batch runs as stream sub-batches, their workspaces as disjoint slices of the same memory
        # (run() and the whole-batch diagnostics are never in flight together)
        K = int(streams)
        sub = K > 1 and B >= 2 * K and T_p and x_sup is None
        bounds = np.linspace(0, B, K + 1).astype(int) if sub else np.array([0, B])
        sub_dims = [_lib.Dims(int(b1 - b0), self.n_tx, n_rx, P, T_p, T_d, self.M, int(partition_r),
                              self.varn, float(varx)) for b0, b1 in zip(bounds[:-1], bounds[1:])]
        sub_bytes = [(_lib.workspace_bytes(d, self.solve) + 255) // 256 * 256 for d in sub_dims]
        whole = _lib.workspace_bytes(self.dims, self.solve)
        self.ws_all = torch.empty(max(whole, sum(sub_bytes) if sub else 0, 16), dtype=torch.uint8,
                                  device="cuda")
        self.ws = self.ws_all[:max(whole, 16)]
        self.x_d = _cdev(torch, x_d_true)
        self.es_table = _linear_es(torch, batch["cons"], None)   # detect_linear's default prior
        self.mom =torch.zeros((B, T_d, self.n_tx + self.n_tx ** 2), dtype=torch.complex128,
                               device="cuda")
        self.x_sup = _cdev(torch, x_sup)
        self.prior = _Prior(*_prior_arg(torch, prior_llr, labels, B, T_d, self.n_tx, self.M, mode))
        if self.prior.opts is not None and int(streams) > 1:
            raise ValueError("prior_llr runs on one stream (sbce_em_multi takes no prior)")
        if early_stop and self.h is None:
            raise ValueError("early_stop needs the true channel (h_true or batch['h'])")
        self.early_stop = bool(early_stop)
        hp = self.h if self.early_stop else None
        self.ptrs = st.ptrs(ws=self.ws, h_true=hp, x_sup=self.x_sup)
        self.subs = []
        self._minnorm_ws = False        # the workspace holds a whole-batch min-norm M-step
        if sub:
            off = 0
            for (b0, b1), dims, nb in zip(zip(bounds[:-1], bounds[1:]), sub_dims, sub_bytes):
                ws = self.ws_all[off:off + nb]
                off += nb
                ptrs = st.ptrs(slice(int(b0), int(b1)), ws=ws, h_true=hp)
                self.subs.append((dims, ptrs, ws, torch.cuda.Stream()))
            # sbce_em_multi's argument arrays over the sub-batches
            n = len(self.subs)
            self._multi = (
                (ctypes.POINTER(_lib.Dims) * n)(*[ctypes.pointer(s[0]) for s in self.subs]),
                (ctypes.POINTER(_lib.Ptrs) * n)(*[ctypes.pointer(s[1]) for s in self.subs]),
                (ctypes.c_void_p * n)(*[s[3].cuda_stream for s in self.subs]),
                (ctypes.c_int * n)())
        # iterations the last run() enqueued per sub-batch (empty without sub-batches)
        self.iters_issued = []

    def run(self, itera, stream=None):
        """One full EM (itera iterations) over the whole batch, stream-ordered on `stream`
        (default: the current stream)."""
        # with stream sub-batches the workspace holds their layouts, not the whole batch's
        self._minnorm_ws = not self.subs and self.solve == _lib.SBCE_SOLVE_MINNORM
        cur = self.torch.cuda.current_stream() if stream is None else stream
        with self.torch.cuda.stream(cur):
            self.theta.copy_(self.theta0)
        if not self.subs and self.prior.opts is not None:
            rc = self.lib.sbce_em_prior(self.dims, self.ptrs, int(itera), self.mode, self.solve,
                                        self.prior.ref(), None, None, cur.cuda_stream)
            _lib.check(rc, "sbce_em_prior")
            return self.theta
        if not self.subs:
            rc = self.lib.sbce_em(self.dims, self.ptrs, int(itera), self.mode, self.solve,
                                  cur.cuda_stream)
            _lib.check(rc, "sbce_em")
            return self.theta
        ev = self.torch.cuda.Event()
        ev.record(cur)
        for _, _, _, st in self.subs:
            st.wait_event(ev)
        dims, ptrs, streams, issued = self._multi
        _lib.check(self.lib.sbce_em_multi(len(self.subs), dims, ptrs, int(itera), self.mode,
                                          self.solve, streams, 0, issued), "sbce_em_multi")
        self.iters_issued = list(issued)
        for _, _, _, st in self.subs:
            cur.wait_stream(st)
        return self.theta

    def capture(self, itera, stream=None):
        """run(itera) captured as ONE HIP graph (stream capture through torch.cuda.CUDAGraph; the
        library's launches on the capturing stream are recorded like torch's own).  sbce_em's
        launch sequence is fixed by the shapes -- the early stop and the sphere pass's work lists
        are device-side -- so ``graph.replay()`` (on the current stream) reruns the whole EM on
        this engine's buffers: one host launch instead of ~4 per iteration, for the sweep grids'
        many small calls, which are host-launch-bound otherwise.  Call run() once before (the
        first launch of each kernel loads its code object)."""
        torch = self.torch
        g = torch.cuda.CUDAGraph()
        side = stream if stream is not None else torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=side):
            self.run(itera)
        torch.cuda.current_stream().wait_stream(side)
        return g

    def estep(self):
        """One E-step launch over the batch from the current theta (for kernel timing)."""
        rc = self.lib.sbce_estep_prior(self.dims, self.ptrs, self.mode, self.prior.ref(),
                                       self.mom.data_ptr(),
                                       self.torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "sbce_estep")

    def mstep(self):
        """One M-step launch sequence from the last E-step moments (for kernel timing)."""
        rc = self.lib.sbce_mstep(self.dims, self.ptrs, self.mom.data_ptr(), self.solve, None,
                                 None, self.torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "sbce_mstep")
        self._minnorm_ws = self.solve == _lib.SBCE_SOLVE_MINNORM

    @property
    def lib(self):
        """libsbce.so -- or libsbce_ab.so inside _lib.debug_env() (A/B and counter runs on the
        same device state: one C-ABI, the workspace carve is the same code)."""
        return _lib.load()

    def mstep_phase(self, phase):
        """One piece of the M-step from the last moments (kernel timing, sbce_debug_mstep_phase):
        0 pilot factorisation, 1 the R build kernel alone, 2 R and B^H."""
        self._minnorm_ws = False                       # R (where G lives) is rebuilt
        fn = self.lib.sbce_debug_mstep_phase
        fn.restype = ctypes.c_int
        rc = fn(ctypes.byref(self.dims), ctypes.byref(self.ptrs), ctypes.c_void_p(self.mom.data_ptr()),
                int(phase), ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "sbce_debug_mstep_phase")

    def detect(self, labels=None, x_d_true=None, noise="em", maxlog=False, want=_WANT,
               return_device=False):
        """One sbce_detect on the engine's resident y_d, psi_d, cons and CURRENT theta (after
        run(): the estimate; before: theta0), on the current stream: the outputs of detect_batch.
        x_d_true defaults to the engine's own (error counters when it has one)."""
        torch = self.torch
        xd = self.x_d if x_d_true is None else _cdev(torch, x_d_true)
        lab = _detect_labels(self.M, labels, "llr" in want or xd is not None)
        lab_d = torch.from_numpy(lab).to("cuda") if lab is not None else None
        s2, s2t = _sigma2_arg(torch, (self.varn, self.varn_t), self.B, noise)
        out = _detect_call(torch, self.y_d, self.psi_d, self.cons, self.theta, self.n_tx, s2, s2t,
                           lab_d, xd, maxlog, tuple(want))
        return _result(torch, out, return_device)

    def detect_linear(self, kind="mmse", es=None, labels=None, x_d_true=None, noise="em",
                      maxlog=False, want=_WANT_LINEAR, return_device=False, ep_passes=None):
        """One sbce_detect_linear on the engine's resident y_d, psi_d, cons and CURRENT theta, on
        the current stream: the outputs of detect_linear_batch (n_tx up to 8).  x_d_true defaults
        to the engine's own.  An engine made with prior_llr passes it on to kind 'ep' (with the
        engine's labelling; ``labels`` must then be left out)."""
        torch = self.torch
        xd = self.x_d if x_d_true is None else _cdev(torch, x_d_true)
        la = None
        if self.prior.opts is not None and (kind[0] if isinstance(kind, tuple) else kind) == "ep":
            if labels is not None:
                raise ValueError("the engine's prior_llr come with the engine's labels")
            la, lab_d = self.prior.la, self.prior.lab
        else:
            lab = _detect_labels(self.M, labels, "llr" in want or xd is not None)
            lab_d = torch.from_numpy(lab).to("cuda") if lab is not None else None
        s2, s2t = _sigma2_arg(torch, (self.varn, self.varn_t), self.B, noise)
        out = _detect_linear_call(torch, self.y_d, self.psi_d, self.cons, self.theta, self.n_tx,
                                  kind, s2, s2t, self.es_table if es is None else float(es), lab_d,
                                  xd, maxlog, tuple(want), ep_passes, la=la)
        return _result(torch, out, return_device)

    def nmse(self):
        """Per-trial NMSE of the current theta against h (device, sbce_nmse)."""
        return nmse_batch(self.theta, self.h)

    def crb(self, kind="em", sigma2=None, want=_WANT_CRB, return_device=False):
        """One sbce_crb on the engine's resident buffers (crb_batch's outputs; the workspace's R is
        overwritten, theta is not).  kind: "em" -- the moments of one E-step (the engine's mode) at
        the CURRENT theta, left in ``self.mom``: the complete-data error variance of the estimate
        the next M-step would make, a truth-free and optimistic predictor of its error; "genie" --
        all data known (needs x_d_true); "pilot" -- pilots only.  sigma2: the noise variance the
        data carry, one value or (B,); default the engine's varn (per trial when it has them).
        ``bound`` is returned when the engine holds the true channel."""
        torch = self.torch
        if kind == "em":
            self.estep()
            mom = self.mom
        elif kind == "genie":
            if self.x_d is None:
                raise ValueError("crb('genie') needs the engine's x_d_true")
            x = self.x_d.reshape(self.B, self.T_d, self.n_tx)
            S = x[..., :, None] * x[..., None, :].conj()
            mom = torch.cat([x, S.reshape(self.B, self.T_d, -1)], dim=2).contiguous()
        elif kind == "pilot":
            mom = torch.zeros_like(self.mom)
        else:
            raise ValueError(f"crb: unknown kind {kind!r}")
        if sigma2 is None:
            s2, s2t = self.varn, self.varn_t
        else:
            s2, s2t = _varn_arg(torch, sigma2, self.B)
        ptrs = _lib.Ptrs.from_buffer_copy(self.ptrs)
        if self.h is not None:
            ptrs.h_true = self.h.data_ptr()
        self._minnorm_ws = False                       # R is rebuilt
        out = _crb_call(torch, self.lib, self.dims, ptrs, mom, s2, s2t, self.h is not None,
                        tuple(want))
        out["status"] = self.status
        if return_device:
            return out
        torch.cuda.current_stream().synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def minnorm_rank(self):
        """(B, 3) int32: active extent, rank of G and whether the refinement step ran, of the
        last whole-batch min-norm M-step (sbce_debug_minnorm_rank; solve='lstsq' only)."""
        if not self._minnorm_ws:
            raise RuntimeError("minnorm_rank: the workspace does not hold a whole-batch min-norm "
                               "M-step (call mstep() with solve='lstsq' first; a streamed run() or "
                               "mstep_phase() overwrites it)")
        out = self.torch.zeros((self.B, 3), dtype=self.torch.int32, device="cuda")
        fn = self.lib.sbce_debug_minnorm_rank
        fn.restype = ctypes.c_int
        rc = fn(ctypes.byref(self.dims), ctypes.byref(self.ptrs), ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "sbce_debug_minnorm_rank")
        return out.cpu().numpy()
