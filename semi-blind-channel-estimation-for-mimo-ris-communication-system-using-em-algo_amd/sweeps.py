"""Monte-Carlo sweep drivers: the reference's entry-point scripts, running the GPU
estimator with every trial of a sweep point batched into ONE sbce_em call.

  nmse_vs_tp   "Proposed method/Proposed_method_NMSEvsTp.py":133-176
  nmse_vs_td   "Proposed method/Proposed_method_NMSEvsTd.py":121-157
  nmse_vs_snr  "Proposed method/SNR/all_Detectors.py":331-395 (its five EMs: PM r=1, log-max,
               ZF, MMSE, exact)
  ser_vs_snr   "Proposed method/SER/log_max_SER.py":124-167 (log-max EM decisions)
  detection_vs_snr  SER / BER / NMSE per SNR of ONE detector (sbce_detect) fed the channel of
               every estimator, the pilot-only start and the true channel, on the data of
               SNR/all_Detectors.py (gen_snr)
  noise_est_vs_snr  NMSE per SNR of the EM with the generating noise parameter, with a fixed wrong
               one and with the parameter estimated from the data (sbce_em_noise), on gen_snr's data
  convergence_vs_snr  NMSE and iterations performed per SNR of a fixed iteration count, the
               truth-free stop (sbce_em_conv) and the oracle stop, on gen_snr's data
  nmse_vs_tp_superimposed  "Parallel/ParallelProtocol_Tp.py":106-136 (superimposed pilots)
  nmse_vs_tp_gaussian      "Proposed method/MIMO_Gaussian_proposed.py":158-177 (Gaussian prior)
  nmse_grid_detectors      "Proposed method/all_detectorsvsTd.py":345-405 (five EMs per T_d
                           point), extended over an SNR axis (BASELINE configs[4])
  llf_vs_iteration         "Proposed method/IterationsvsLLF.py":119-157 (LLF per EM iteration)
  comparison_vs_td         "Comparision/Comparision T_d vs NMSE.py":203-253 and
  comparison_vs_tp         "Comparision/Comparision T_p .py":171-222: the proposed exact EM beside
                           the semi-blind Gaussian-approximation EM (EM_approx), the figure
                           "Comparison between proposed method and the semi-blind Gaussian
                           method"; per point one sbce_approx_em call over every trial (one kernel
                           launch, csrc/approx.hip) and the proposed leg's sbce_em calls

Data generation (host, NumPy):
  replay=True   the reference's exact legacy-RandomState call order after
                np.random.seed(seed) (trials generated sequentially, so every rank
                replays the whole stream and keeps its own trials);
  replay=False  per-trial numpy Generators seeded (seed, trial): statistical parity,
                no sequential dependence (large sweeps / many GPUs).
Multi-GPU: when torch.distributed is initialised, trials are sharded
(distributed.shard) and the per-point accumulators are all-reduced ONCE at the end.
"""
import numpy as np

from . import signal_model as sm
from .distributed import Accumulators, shard
from .em import (em_batch, em_approx_batch, ser_batch, gauss_expand_batch, nmse_batch,
                 detect_batch, detect_linear_batch, em_batch_noise, em_batch_conv, _GAUSS_CONS,
                 crb_batch)
from .qam import qam_constellation, gray_labeling


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_world_size(), dist.get_rank()
    except ImportError:
        pass
    return None, 1, 0


def _trial_rng(seed, trial):
    return np.random.RandomState(np.random.SeedSequence([seed, trial]).generate_state(1)[0])


def _pack(trials, P):
    """Stack per-trial dicts into the batch-major C-ABI arrays."""
    return dict(
        y_d=np.stack([t["Y_d"] for t in trials]),
        y_p=np.stack([t["Y_p"] for t in trials]),
        psi_d=np.stack([t["Psi_d"].T for t in trials]),
        u_p=np.stack([t["U_p"] for t in trials]),
        theta0=np.stack([t["h0"] for t in trials]),
        h=np.stack([t["h"] for t in trials]),
    )


def _nmse(theta, h):
    return np.sum(np.abs(theta - h) ** 2, axis=1) / np.sum(np.abs(h) ** 2, axis=1)


def _run_points(points, cons, varns, itera, mode, acc, dist):
    for pt, (trials, varn) in enumerate(zip(points, varns)):
        if not trials:
            continue
        b = _pack(trials, None)
        r = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, varn, itera, b["theta0"],
                     mode=mode)
        acc.add(pt, _nmse(r["theta"], b["h"]))
    return acc


def nmse_vs_tp(T_p=(4, 12, 20, 28, 36, 40), T_d=50, N=32, n_rx=4, n_tx=4, itera=3, monte_iter=1,
               M=4, varn=0.1, seed=0, replay=True, mode="soft", varh=1.0):
    """Mean NMSE per pilot length (PMd/Proposed_method_NMSEvsTp.py:154-176).

    Reference draw order per trial: channelMatrix, symbols(T_d), pilotSymbols(max T_p),
    then for each T_p: irsMatrix (T_d uniform draws), receivedSignals (noise)."""
    dist, world, rank = _dist()
    mine = set(shard(monte_iter, world, rank).tolist())
    points = [[] for _ in T_p]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in mine:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, rs=rs)
        X_d, _ = sm.symbols(n_tx, M, T_d, rs=rs)
        X_p = sm.pilot_symbols(n_tx, M, max(T_p), rs=rs)
        for k, tp in enumerate(T_p):
            Ptp, Ptd = sm.irs_matrix(tp, T_d, N, rs=rs)
            Ptd = sm.insert_direct(Ptd)
            Y_p, Y_d, U_p, _, h0 = sm.received_signals(tp, T_d, Ptp, Ptd, n_rx, n_tx, X_d, X_p[:tp],
                                                       h, varn, rs=rs)
            if i in mine:
                points[k].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h))
    acc = Accumulators(len(T_p))
    _run_points(points, qam_constellation(M), [varn] * len(T_p), itera, mode, acc, dist)
    acc.allreduce(dist)
    return np.asarray(T_p), acc.mean_nmse()


def nmse_vs_td(T_d=(20, 30, 40, 50, 60, 70, 80, 90, 100), T_p=16, N=32, n_rx=2, n_tx=2, itera=3,
               monte_iter=1, M=4, varn=0.1, seed=0, replay=True, mode="soft", varh=1.0,
               variant="pmd"):
    """Mean NMSE per data length (PMd/Proposed_method_NMSEvsTd.py:140-157; C-order h, :15).

    Reference draw order per trial: channelMatrix, pilotSymbols(T_p), then for each T_d:
    symbols(T_d), irsMatrix, receivedSignals.
    variant='root': the root-level Proposed_method_NMSEvsTd.py -- the same draw order, N x T_p
    DFT pilot phases over T_p plus a ones row (:81-86, :95), deterministic (N+1) x T_d DFT data
    phases over T_d (:92-94, no RNG draw: signal_model.irs_matrix(data='dft_td')) and the EM
    started from theta = 0 (:46, em_zero_init)."""
    if variant not in ("pmd", "root"):
        raise ValueError(variant)
    root = variant == "root"
    dist, world, rank = _dist()
    mine = set(shard(monte_iter, world, rank).tolist())
    points = [[] for _ in T_d]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in mine:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, order="C", rs=rs)
        X_p = sm.pilot_symbols(n_tx, M, T_p, rs=rs)
        for k, td in enumerate(T_d):
            X_d, _ = sm.symbols(n_tx, M, td, rs=rs)
            if root:
                Ptp, Ptd = sm.irs_matrix(T_p, td, N, pilot="dft_tp", data="dft_td", rs=rs)
                Ptp = sm.insert_direct(Ptp)
            else:
                Ptp, Ptd = sm.irs_matrix(T_p, td, N, rs=rs)
            Ptd = sm.insert_direct(Ptd)
            Y_p, Y_d, U_p, _, h0 = sm.received_signals(T_p, td, Ptp, Ptd, n_rx, n_tx, X_d, X_p, h,
                                                       varn, rs=rs, with_initial=not root)
            if root:
                h0 = np.zeros(len(h), dtype=complex)
            if i in mine:
                points[k].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h))
    acc = Accumulators(len(T_d))
    _run_points(points, qam_constellation(M), [varn] * len(T_d), itera, mode, acc, dist)
    acc.allreduce(dist)
    return np.asarray(T_d), acc.mean_nmse()


def gen_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=12, N=10, n_rx=2, n_tx=2, monte_iter=15, M=4,
            power=10.0, seed=0, replay=True, varh=1.0, keep=None):
    """Synthetic data of PMd/SNR/all_Detectors.py:362-370 in the reference draw order:
    per trial channelMatrix, symbols, pilotSymbols, irsMatrix once, then per SNR
    receivedSignals.  Returns (points, varns): points[k] = list of per-trial dicts."""
    varns = sm.snr_to_varn(SNR, power)
    keep = set(range(monte_iter)) if keep is None else set(keep)
    points = [[] for _ in SNR]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, rs=rs)
        X_d, _ = sm.symbols(n_tx, M, T_d, rs=rs)
        X_p = sm.pilot_symbols(n_tx, M, T_p, rs=rs)
        Ptp, Ptd = sm.irs_matrix(T_p, T_d, N, rs=rs)
        Ptd = sm.insert_direct(Ptd)
        for k in range(len(SNR)):
            Y_p, Y_d, U_p, _, h0 = sm.received_signals(T_p, T_d, Ptp, Ptd, n_rx, n_tx, X_d, X_p, h,
                                                       varns[k], rs=rs)
            if i in keep:
                points[k].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h,
                                      X_d=np.stack([x.reshape(-1) for x in X_d])))
    return points, varns


# The five EMs of the NMSE-vs-SNR figure, PMd/SNR/all_Detectors.py:372-377, in the script's call
# order: (E-step mode, reference EM, oracle early stop on the true h as THIS script has it, plot
# label :396-401).  Unlike all_detectorsvsTd.py (DETECTORS below, every EM stops), only em_pm
# stops here (:234-236); em_zf's stop is commented out (:125-127); em_mmse, em_ml, em have none.
SNR_DETECTORS = {
    "pm_soft": ("em_pm :170-240 (posterior-weighted list, partition_r_1 = 1)", True,
                "Soft decision-PM r =1"),
    "hard": ("em_ml :132-167 (log-max)", False, "log-max"),
    "zf": ("em_zf :92-130", False, "Zero forcing"),
    "mmse": ("em_mmse :53-90", False, "MMSE"),
    "soft": ("em :242-274 (exact posterior)", False, "Exact"),
    # not in the reference: the soft E-steps for up to 8 streams (em.em_mmse_soft / em_zf_soft);
    # selectable by name, not part of the default figure
    "mmse_soft": ("soft MMSE (no reference counterpart)", False, "Soft MMSE"),
    "zf_soft": ("soft ZF (no reference counterpart)", False, "Soft ZF"),
    # expectation propagation on the soft MMSE solve (em.em_ep), default pass count
    "ep": ("expectation propagation (no reference counterpart)", False, "EP"),
}
# the reference figure's five EMs: the default of nmse_vs_snr
SNR_DEFAULT_MODES = ("pm_soft", "hard", "zf", "mmse", "soft")


def _snr_groups(points, varns, batch_snr):
    """The sbce_em calls of an SNR axis: with batch_snr ONE call over the trials of every SNR
    point (per-trial noise variances, include/sbce.h sbce_ptrs.varn_t), else one call per point.
    Yields (SNR indices, trials per index, packed batch, varn scalar or (B,) array)."""
    live = [k for k, t in enumerate(points) if t]
    if not live:
        return
    if batch_snr and len(live) > 1:
        trials = [t for k in live for t in points[k]]
        vt = np.concatenate([np.full(len(points[k]), varns[k]) for k in live])
        yield live, [len(points[k]) for k in live], _pack(trials, None), vt
    else:
        for k in live:
            yield [k], [len(points[k])], _pack(points[k], None), varns[k]


def nmse_vs_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=12, N=10, n_rx=2, n_tx=2, itera=5,
                monte_iter=15, M=4, power=10.0, seed=0, replay=True, modes=SNR_DEFAULT_MODES,
                varh=1.0, partition_r=1, return_status=False, batch_snr=True, bounds=False):
    """Mean NMSE per SNR of the five EMs of PMd/SNR/all_Detectors.py (driver :362-395; varn =
    power / 10^(SNR/10), :351-354): em_pm (r = 1), em_ml, em_zf, em_mmse and the exact em, each
    with that script's own early-stop pattern (SNR_DETECTORS) and np.linalg.solve M-step.
    modes may also name "mmse_soft" / "zf_soft" / "ep" (the soft E-steps for n_tx up to 8, which
    the reference does not have); pm_soft, zf and mmse take n_tx up to 8 too, hard and soft up to 4.

    One batched sbce_em per detector over this rank's trials of EVERY SNR point (per-trial noise
    variances; batch_snr=False: one call per (SNR point, detector), the same results); the
    accumulators of every (detector, SNR) point are all-reduced ONCE at the end.  Returns (SNR, {mode: curve});
    with return_status also {mode: (len(SNR),) count of trials whose status word is non-zero
    (e.g. SBCE_STATUS_DETECTOR: the reference's nearest_symbol_ecul would raise IndexError)}.

    bounds=True: the curves also carry "crb_genie", the mean over trials of the Cramer-Rao bound on
    the NMSE with all data known (em.crb_batch kind "genie", sigma2 = the point's varn): the floor
    the semi-blind curves approach at high SNR.  It rides in the same accumulators and the one
    all-reduce; it is +inf when any trial of the point is unidentifiable (T_p + T_d < L), and
    return_status then also counts those trials under "crb_genie"."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_snr(SNR, T_d, T_p, N, n_rx, n_tx, monte_iter, M, power, seed, replay,
                            varh, keep=mine)
    cons = qam_constellation(M)
    nm, ns = len(modes), len(SNR)
    acc = Accumulators(nm * ns + (ns if bounds else 0), n_extra=1)
    if bounds:
        for k, trials in enumerate(points):
            if not trials:
                continue
            b = _pack(trials, None)
            r = crb_batch(None, None, b["psi_d"], b["u_p"], cons, n_tx, varns[k], kind="genie",
                          x_d_true=np.stack([t["X_d"] for t in trials]), h_true=b["h"],
                          want=("tr_inv",))
            acc.add(nm * ns + k, r["bound"],
                    extra_values=(r["status"] != 0).astype(float)[:, None])
    for ks, counts, b, vn in _snr_groups(points, varns, batch_snr):
        for mi, mode in enumerate(modes):
            stop = SNR_DETECTORS[mode][1]
            r = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, vn, itera,
                         b["theta0"], mode=mode,
                         partition_r=partition_r if mode.startswith("pm") else 0,
                         h_true=b["h"] if stop else None)
            err, flag = _nmse(r["theta"], b["h"]), (r["status"] != 0).astype(float)[:, None]
            off = np.cumsum([0] + counts)
            for k, o0, o1 in zip(ks, off[:-1], off[1:]):
                acc.add(mi * ns + k, err[o0:o1], extra_values=flag[o0:o1])
    acc.allreduce(dist)                   # the sweep's only collective
    mean = acc.mean_nmse()[:nm * ns].reshape(nm, ns)
    curves = {mode: mean[mi] for mi, mode in enumerate(modes)}
    if bounds:
        curves["crb_genie"] = acc.mean_nmse()[nm * ns:]
    if return_status:
        flagged = acc.extra[:nm * ns, 0].reshape(nm, ns)
        status = {mode: flagged[mi] for mi, mode in enumerate(modes)}
        if bounds:
            status["crb_genie"] = acc.extra[nm * ns:, 0]
        return np.asarray(SNR), curves, status
    return np.asarray(SNR), curves


NOISE_CURVES = ("known", "assumed", "estimated")


def noise_est_vs_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=12, N=10, n_rx=2, n_tx=2, itera=8,
                     monte_iter=15, M=4, varn_assumed=1.0, power=10.0, seed=0, replay=True,
                     mode="soft", varh=1.0, varn_min=1e-6, batch_snr=True):
    """What estimating the noise parameter is worth, per SNR, on gen_snr's data (the layout of
    PMd/SNR/all_Detectors.py:362-370): the mean NMSE of the EM run with
      'known'     the generating varn as its parameter (em_batch),
      'assumed'   the fixed wrong parameter varn_assumed (em_batch),
      'estimated' the parameter estimated from the data, started at varn_assumed (em_batch_noise),
    and the mean of sigma_hat^2 / sigma_true^2 of the third (sigma_true^2 = varn, the variance the
    noise was drawn with; sigma_hat^2 = the estimate's ``sigma2``).
    Trials shard over ranks as in nmse_vs_snr; the SNR axis rides in one call per curve through
    per-trial parameters (batch_snr=False: one call per point, the same results); the accumulators
    are all-reduced ONCE.  Returns (SNR, {curve: NMSE per SNR}, ratio per SNR)."""
    if not varn_assumed > 0:
        raise ValueError("varn_assumed must be > 0")
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_snr(SNR, T_d, T_p, N, n_rx, n_tx, monte_iter, M, power, seed, replay,
                            varh, keep=mine)
    cons = qam_constellation(M)
    nc, ns = len(NOISE_CURVES), len(SNR)
    acc = Accumulators(nc * ns, n_extra=1)
    for ks, counts, b, vn in _snr_groups(points, varns, batch_snr):
        args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons)
        vt = np.broadcast_to(np.asarray(vn, dtype=float), (len(b["h"]),))
        known = em_batch(*args, vn, itera, b["theta0"], mode=mode)
        fixed = em_batch(*args, float(varn_assumed), itera, b["theta0"], mode=mode)
        est = em_batch_noise(*args, float(varn_assumed), itera, b["theta0"], mode=mode,
                             varn_min=varn_min)
        ratio = (np.asarray(est["sigma2"]) / vt)[:, None]
        off = np.cumsum([0] + counts)
        for ci, r in enumerate((known, fixed, est)):
            err = _nmse(np.asarray(r["theta"]), b["h"])
            for k, o0, o1 in zip(ks, off[:-1], off[1:]):
                acc.add(ci * ns + k, err[o0:o1], extra_values=ratio[o0:o1] if ci == 2 else None)
    acc.allreduce(dist)                   # the sweep's only collective
    mean = acc.mean_nmse().reshape(nc, ns)
    ratio = acc.mean_extra()[:, 0].reshape(nc, ns)[2]
    return np.asarray(SNR), {c: mean[i] for i, c in enumerate(NOISE_CURVES)}, ratio


CONV_ARMS = ("fixed", "stop", "oracle")


def convergence_vs_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=12, N=10, n_rx=2, n_tx=2, itera=20,
                       monte_iter=15, M=4, tol_theta=1e-6, min_iters=2, power=10.0, seed=0,
                       replay=True, mode="soft", varh=1.0, batch_snr=True):
    """What a stop rule costs and saves, per SNR, on gen_snr's data: the mean NMSE and the mean
    number of iterations performed of the EM run with
      'fixed'   the fixed count itera (em_batch),
      'stop'    the truth-free stop ||theta_l - theta_{l-1}|| <= tol_theta ||theta_l||, at most
                itera iterations (em_batch_conv),
      'oracle'  the reference's oracle stop | ||theta|| - ||h|| | < 1 on the true channel
                (em_batch with h_true, PM.py:110-112), at most itera iterations.
    Trials shard over ranks as in nmse_vs_snr; the SNR axis rides in one call per arm through
    per-trial parameters (batch_snr=False: one call per point, the same results); the accumulators
    are all-reduced ONCE.  Returns (SNR, {arm: NMSE per SNR}, {arm: mean iterations per SNR})."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_snr(SNR, T_d, T_p, N, n_rx, n_tx, monte_iter, M, power, seed, replay,
                            varh, keep=mine)
    cons = qam_constellation(M)
    na, ns = len(CONV_ARMS), len(SNR)
    acc = Accumulators(na * ns, n_extra=1)
    for ks, counts, b, vn in _snr_groups(points, varns, batch_snr):
        args = (b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, vn, itera, b["theta0"])
        runs = (em_batch(*args, mode=mode),
                em_batch_conv(*args, tol_theta=tol_theta, min_iters=min_iters, mode=mode),
                em_batch(*args, mode=mode, h_true=b["h"]))
        off = np.cumsum([0] + counts)
        for ai, r in enumerate(runs):
            err = _nmse(np.asarray(r["theta"]), b["h"])
            its = np.asarray(r["iters_done"], dtype=float)[:, None]
            for k, o0, o1 in zip(ks, off[:-1], off[1:]):
                acc.add(ai * ns + k, err[o0:o1], extra_values=its[o0:o1])
    acc.allreduce(dist)                   # the sweep's only collective
    mean = acc.mean_nmse().reshape(na, ns)
    its = acc.mean_extra()[:, 0].reshape(na, ns)
    return (np.asarray(SNR), {a: mean[i] for i, a in enumerate(CONV_ARMS)},
            {a: its[i] for i, a in enumerate(CONV_ARMS)})


def gen_ser(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=20, N=30, n_rx=2, n_tx=2, monte_iter=75, M=4,
            power=10.0, seed=0, replay=True, varh=1.0, keep=None):
    """Synthetic data of PMd/SER/log_max_SER.py:150-160 in the reference draw order: per
    trial channelMatrix, symbols(T_d), irsMatrix (pilot phases (N+1) x T_p with a zero last
    row; ones row inserted into the data phases), pilotSymbols, then per SNR
    receivedSignals."""
    varns = sm.snr_to_varn(SNR, power)
    keep = set(range(monte_iter)) if keep is None else set(keep)
    points = [[] for _ in SNR]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, rs=rs)
        X_d, _ = sm.symbols(n_tx, M, T_d, rs=rs)
        Ptp, Ptd = sm.irs_matrix(T_p, T_d, N, pilot="dft_n", rs=rs)
        Ptd = sm.insert_direct(Ptd)
        X_p = sm.pilot_symbols(n_tx, M, T_p, rs=rs)
        for k in range(len(SNR)):
            Y_p, Y_d, U_p, _, h0 = sm.received_signals(T_p, T_d, Ptp, Ptd, n_rx, n_tx, X_d, X_p, h,
                                                       varns[k], rs=rs)
            if i in keep:
                points[k].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h,
                                      X_d=np.stack([x.reshape(-1) for x in X_d])))
    return points, varns


def ser_vs_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=20, N=30, n_rx=2, n_tx=2, itera=5,
               monte_iter=75, M=4, power=10.0, seed=0, replay=True, varh=1.0):
    """SER per SNR of the log-max EM's last-iteration decisions (PMd/SER/log_max_SER.py:
    constants :124-147, driver :150-167).  Returns (SNR, ser_reference, ser_elementwise,
    nmse): ser_reference is the script's own expression (:162, a (T_d, n_tx, n_tx)
    broadcast count), ser_elementwise the per-symbol-entry error rate.

    Reference draw order per trial: channelMatrix, symbols(T_d), irsMatrix (ones row
    inserted, pilot phases (N+1) x T_p with a zero last row), pilotSymbols, then per SNR
    receivedSignals (gen_ser)."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_ser(SNR, T_d, T_p, N, n_rx, n_tx, monte_iter, M, power, seed, replay,
                            varh, keep=mine)
    acc = Accumulators(len(SNR), n_extra=2)
    cons = qam_constellation(M)
    for pt, trials in enumerate(points):
        if not trials:
            continue
        b = _pack(trials, None)
        r = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, varns[pt], itera,
                     b["theta0"], mode="hard", return_decisions=True)
        x_true = np.stack([t["X_d"] for t in trials])
        s_ref, s_el = ser_batch(r["x_dest"], x_true)
        acc.add(pt, _nmse(r["theta"], b["h"]), extra_values=np.stack([s_ref, s_el], axis=1))
    acc.allreduce(dist)
    ser = acc.mean_extra()
    return np.asarray(SNR), ser[:, 0], ser[:, 1], acc.mean_nmse()


# channel fed to the detector: the pilot-only start h0, the true channel, or em_batch's theta
DETECT_ESTIMATORS = ("pilot", "soft", "hard", "pm", "zf", "mmse", "genie")


def detection_vs_snr(SNR=(-5, 0, 5, 10, 15, 20), T_d=50, T_p=12, N=10, n_rx=2, n_tx=2, itera=5,
                     monte_iter=15, M=4, estimators=DETECT_ESTIMATORS, power=10.0, seed=0,
                     replay=True, varh=1.0, partition_r=1, noise="em", labels=None,
                     batch_snr=True, detector="ml"):
    """Uncoded SER and BER (and NMSE) per SNR of the joint ML detector (sbce_detect) fed each
    estimator's channel, on gen_snr's data (the layout of PMd/SNR/all_Detectors.py:362-370):
    'pilot' = the pilot-only start h0, 'genie' = the true h, every other name an em_batch mode
    (soft, hard, pm, pm_soft, zf, mmse, mmse_soft, zf_soft, ep) whose theta after ``itera`` iterations
    is used.  The SAME detector serves every estimator;
    per-trial symbol and bit error counts come from the device counters and are accumulated as
    extras, all-reduced ONCE with the NMSE sums.  noise: the detector's sigma^2 ('em' varn^2,
    'true' varn); labels: the bit labelling (default qam.gray_labeling).
    detector: 'ml' (sbce_detect, n_tx <= 4), or the linear receivers 'mmse' / 'zf' / 'ep'
    (sbce_detect_linear, prior energy mean |cons|^2; 'ep' with its default pass count), which take
    n_tx up to 8 with the estimators pilot, genie, pm, pm_soft, zf, mmse, mmse_soft, zf_soft and ep; soft and hard keep the exact
    E-step's own limit
    (n_tx <= 4, M^n_tx <= 2^24) and raise ValueError beyond it.
    Returns (SNR, ser {est: curve}, ber {est: curve}, nmse {est: curve})."""
    estimators = tuple(estimators)
    bad = [e for e in estimators if e not in ("pilot", "genie", "soft", "hard", "pm", "pm_soft",
                                              "zf", "mmse", "mmse_soft", "zf_soft", "ep")]
    if bad:
        raise ValueError(f"unknown estimators {bad}")
    if detector not in ("ml", "mmse", "zf", "ep"):
        raise ValueError("detector must be 'ml', 'mmse', 'zf' or 'ep'")
    if detector != "ml" and (n_tx > 4 or M ** n_tx > 1 << 24):
        beyond = [e for e in estimators if e in ("soft", "hard")]
        if beyond:
            raise ValueError(f"estimators {beyond} enumerate M^n_tx hypotheses: n_tx <= 4 and "
                             f"M^n_tx <= 2^24 (n_tx = {n_tx}, M = {M})")
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_snr(SNR, T_d, T_p, N, n_rx, n_tx, monte_iter, M, power, seed, replay,
                            varh, keep=mine)
    cons = qam_constellation(M)
    lab = gray_labeling(M) if labels is None else np.asarray(labels, dtype=np.int32)
    ne, ns = len(estimators), len(SNR)
    acc = Accumulators(ne * ns, n_extra=2)
    for ks, counts, b, vn in _snr_groups(points, varns, batch_snr):
        x_true = np.stack([t["X_d"] for k in ks for t in points[k]])
        off = np.cumsum([0] + counts)
        for ei, est in enumerate(estimators):
            if est == "pilot":
                theta = b["theta0"]
            elif est == "genie":
                theta = b["h"]
            else:
                theta = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, vn, itera,
                                 b["theta0"], mode=est,
                                 partition_r=partition_r if est.startswith("pm") else 0)["theta"]
            if detector == "ml":
                r = detect_batch(b["y_d"], b["psi_d"], cons, theta, vn, n_tx, labels=lab,
                                 x_d_true=x_true, noise=noise, want=())
            else:
                r = detect_linear_batch(b["y_d"], b["psi_d"], cons, theta, vn, n_tx,
                                        kind=detector, labels=lab, x_d_true=x_true, noise=noise,
                                        want=())
            nm = _nmse(np.asarray(theta), b["h"])
            for k, o0, o1 in zip(ks, off[:-1], off[1:]):
                acc.add(ei * ns + k, nm[o0:o1], extra_values=r["err"][o0:o1])
    acc.allreduce(dist)                   # the sweep's only collective
    n_sym = np.maximum(acc.count, 1) * (T_d * n_tx)
    lgM = max(int(M - 1).bit_length(), 1)
    ser = (acc.extra[:, 0] / n_sym).reshape(ne, ns)
    ber = (acc.extra[:, 1] / (n_sym * lgM)).reshape(ne, ns)
    nmse = acc.mean_nmse().reshape(ne, ns)
    return (np.asarray(SNR), {e: ser[i] for i, e in enumerate(estimators)},
            {e: ber[i] for i, e in enumerate(estimators)},
            {e: nmse[i] for i, e in enumerate(estimators)})


def gen_superimposed(T_p=(4, 8, 12, 16, 20, 24, 28, 32, 36, 40), T_d=50, N=32, n_rx=8, n_tx=1,
                     monte_iter=50, M=16, varn=0.1, seed=0, replay=True, varh=1.0, keep=None):
    """Data of Parallel/ParallelProtocol_Tp.py:114-122 in the reference draw order: per
    trial channelMatrix (C-order h, :10-16), symbols(T_d); per T_p irsMatrix(T, N)
    ((N+1) x T DFT, deterministic), pilotSymbols, dataPilotSymbols (zero-padded sum),
    receivedSignals (one noise draw per symbol)."""
    keep = set(range(monte_iter)) if keep is None else set(keep)
    points = [[] for _ in T_p]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, order="C", rs=rs)
        X_d, _ = sm.symbols(n_tx, M, T_d, rs=rs)
        for k, tp in enumerate(T_p):
            T = max(T_d, tp)
            Psi = sm.dft_phases(N + 1, T, T)
            X_p = sm.pilot_symbols(n_tx, M, tp, rs=rs)
            xd = np.zeros((T, n_tx), dtype=complex)
            xp = np.zeros((T, n_tx), dtype=complex)
            xd[:T_d] = np.stack([x.reshape(-1) for x in X_d])
            xp[:tp] = np.stack([x.reshape(-1) for x in X_p])
            X = xd + xp
            _, Y, _, _, _ = sm.received_signals(0, T, Psi[:, :0], Psi, n_rx, n_tx, list(X), [], h,
                                                varn, rs=rs, with_initial=False)
            if i in keep:
                points[k].append(dict(Y=Y, Psi=Psi, X_sup=xp, h=h))
    return points


def nmse_vs_tp_superimposed(T_p=(4, 8, 12, 16, 20, 24, 28, 32, 36, 40), T_d=50, N=32, n_rx=8,
                            n_tx=1, itera=20, monte_iter=50, M=16, varn=0.1, seed=0, replay=True,
                            varh=1.0):
    """Mean NMSE per pilot length of the superimposed-pilot protocol
    (Parallel/ParallelProtocol_Tp.py:106-136; NMSE :129)."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points = gen_superimposed(T_p, T_d, N, n_rx, n_tx, monte_iter, M, varn, seed, replay, varh,
                              keep=mine)
    acc = Accumulators(len(T_p))
    cons = qam_constellation(M)
    for k, trials in enumerate(points):
        if not trials:
            continue
        L = (N + 1) * n_tx
        B = len(trials)
        r = em_batch(np.stack([t["Y"] for t in trials]), np.zeros((B, 0, n_rx), dtype=complex),
                     np.stack([t["Psi"].T for t in trials]), np.zeros((B, 0, L), dtype=complex),
                     cons, varn, itera, np.zeros((B, L * n_rx), dtype=complex), mode="soft",
                     x_sup=np.stack([t["X_sup"] for t in trials]))
        acc.add(k, _nmse(r["theta"], np.stack([t["h"] for t in trials])))
    acc.allreduce(dist)
    return np.asarray(T_p), acc.mean_nmse()


def gen_gaussian(T_p=(8, 12, 16, 20, 24, 28, 32, 36, 40), T_d=50, N=32, n_rx=2, n_tx=2,
                 monte_iter=1, varn=0.1, varx=1.0, seed=0, replay=True, varh=1.0, keep=None):
    """Data of MIMO_Gaussian_proposed.py:160-169 in the reference draw order: per trial
    channelMatrix1 and symbols(n_tx, T_d, varx); per T_p irsMatrix (N x T_p DFT + T_d
    uniform phase draws), pilotSymbols, received_proposed (one noise draw per symbol).
    Reduced form: u_p = psi_p (x) x_p, y = H z = H_r u, h_initial = Y_p pinv(Z_p) reduced."""
    keep = set(range(monte_iter)) if keep is None else set(keep)
    points = [[] for _ in T_p]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.gaussian_channel(varh, N, n_rx, n_tx, rs=rs)
        X_d = sm.gaussian_symbols(n_tx, T_d, varx, rs=rs)
        for k, tp in enumerate(T_p):
            Ptp, Ptd = sm.irs_matrix(tp, T_d, N, pilot="dft_n", rs=rs)
            Ptp = Ptp[:N]
            X_p = sm.gaussian_symbols(n_tx, tp, varx, rs=rs)
            Y_p, Y_d, U_p, _, h0 = sm.received_signals(tp, T_d, Ptp, Ptd, n_rx, n_tx, X_d.T,
                                                       X_p.T, h, varn, rs=rs)
            if i in keep:
                points[k].append(dict(Y_d=Y_d, Y_p=Y_p, U_p=U_p, Psi_d=Ptd, h0=h0, h=h))
    return points


def nmse_vs_tp_gaussian(T_p=(8, 12, 16, 20, 24, 28, 32, 36, 40), T_d=50, N=32, n_rx=2, n_tx=2,
                        itera=3, monte_iter=1, varn=0.1, varx=1.0, seed=0, replay=True,
                        varh=1.0):
    """Mean NMSE per pilot length of the Gaussian-prior EM (MIMO_Gaussian_proposed.py:
    158-177): trace(|(H_hat - H)^H (H_hat - H)|) / ||H||^2 (:173) on the full n_rx x Q
    matrices, H_hat = the reference-format expansion of the device estimate."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points = gen_gaussian(T_p, T_d, N, n_rx, n_tx, monte_iter, varn, varx, seed, replay, varh,
                          keep=mine)
    acc = Accumulators(len(T_p))
    for k, trials in enumerate(points):
        if not trials:
            continue
        d = _pack(trials, N)
        r = em_batch(d["y_d"], d["y_p"], d["psi_d"], d["u_p"], _GAUSS_CONS, varn, itera + 1,
                     d["theta0"], mode="gauss", varx=varx, solve="drop", return_device=True)
        Hh = gauss_expand_batch(r["theta"], n_tx, n_rx, return_device=True)
        Hf = np.stack([sm.full_gaussian_channel(h, n_rx).reshape(-1) for h in d["h"]])
        acc.add(k, nmse_batch(Hh.reshape(len(trials), -1), Hf).cpu().numpy())
    acc.allreduce(dist)
    return np.asarray(T_p), acc.mean_nmse()


# (E-step mode, reference EM of all_detectorsvsTd.py, its plot label :407-411)
DETECTORS = {
    "pm_soft": ("em_pm :176-249 (posterior-weighted list, partition_r)", "Soft decision-PM"),
    "hard": ("em_ml :135-173 (log-max)", "Non - Superimposed log-max"),
    "zf": ("em_zf :95-133", "Zero forcing"),
    "mmse": ("em_mmse :54-93", "MMSE"),
    "soft": ("em :260-295 (exact posterior)", "Non - Superimposed"),
}


def gen_detectors(T_d=(15, 30, 45, 60, 75, 90), SNR=None, T_p=20, N=15, n_rx=2, n_tx=2,
                  monte_iter=1, M=4, varn=0.1, power=10.0, seed=0, replay=True, varh=1.0,
                  keep=None):
    """Data of PMd/all_detectorsvsTd.py:371-382 in its draw order: per trial channelMatrix,
    pilotSymbols(T_p); per T_d point symbols(T_d), irsMatrix (pilot phases (N+1) x T_p DFT
    with a zero last row, T_d uniform data-phase columns), the ones row inserted, then
    receivedSignals (h_initial by scipy.linalg.pinv, :341) -- once with the script's varn
    (SNR=None), or once per SNR point in SNR order (the grid extension of BASELINE
    configs[4]; varn = power / 10^(SNR/10), SNR/all_Detectors.py:351-354).  Returns (points[k_td][k_snr] = trial dicts, varns)."""
    varns = [float(varn)] if SNR is None else [float(v) for v in sm.snr_to_varn(SNR, power)]
    keep = set(range(monte_iter)) if keep is None else set(keep)
    points = [[[] for _ in varns] for _ in T_d]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, rs=rs)
        X_p = sm.pilot_symbols(n_tx, M, T_p, rs=rs)
        for k, td in enumerate(T_d):
            X_d, _ = sm.symbols(n_tx, M, td, rs=rs)
            Ptp, Ptd = sm.irs_matrix(T_p, td, N, pilot="dft_n", rs=rs)
            Ptd = sm.insert_direct(Ptd)
            for j, vn in enumerate(varns):
                Y_p, Y_d, U_p, _, h0 = sm.received_signals(T_p, td, Ptp, Ptd, n_rx, n_tx, X_d,
                                                           X_p, h, vn, rs=rs, pinv="scipy")
                if i in keep:
                    points[k][j].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h))
    return points, varns


def nmse_grid_detectors(T_d=(15, 30, 45, 60, 75, 90), SNR=None, T_p=20, N=15, n_rx=2, n_tx=2,
                        itera=5, monte_iter=1, M=4, varn=0.1, power=10.0, partition_r=1, seed=0,
                        replay=True, detectors=tuple(DETECTORS), early_stop=True, varh=1.0,
                        batch_snr=True):
    """Mean NMSE of the five EMs of PMd/all_detectorsvsTd.py (:384-405) per T_d point, and
    per SNR point when SNR is given (BASELINE configs[4]: 20 SNR x 8 T_d, 64-QAM).

    One batched sbce_em per (T_d, detector) over this rank's trials of every SNR point (per-trial
    noise variances; batch_snr=False: one per (T_d, SNR, detector), the same results); every EM
    keeps the script's oracle early stop on the true h (:87-89, :128-130, :169-171, :243-245,
    :291-293) unless early_stop=False, and its np.linalg.solve M-step (SBCE_SOLVE_CHOL).
    The accumulators of the whole grid are all-reduced once.  Returns (T_d, SNR or None,
    {detector: (len(T_d), len(SNR or [varn])) mean NMSE})."""
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    points, varns = gen_detectors(T_d, SNR, T_p, N, n_rx, n_tx, monte_iter, M, varn, power, seed,
                                  replay, varh, keep=mine)
    cons = qam_constellation(M)
    nd, nt, ns = len(detectors), len(T_d), len(varns)
    acc = Accumulators(nd * nt * ns)
    for k in range(nt):
        for js, counts, b, vn in _snr_groups(points[k], varns, batch_snr):
            off = np.cumsum([0] + counts)
            for di, det in enumerate(detectors):
                r = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], cons, vn, itera,
                             b["theta0"], mode=det, partition_r=partition_r if det == "pm_soft" else 0,
                             h_true=b["h"] if early_stop else None)
                nm = _nmse(r["theta"], b["h"])
                for j, o0, o1 in zip(js, off[:-1], off[1:]):
                    acc.add((di * nt + k) * ns + j, nm[o0:o1])
    acc.allreduce(dist)
    mean = acc.mean_nmse().reshape(nd, nt, ns)
    return (np.asarray(T_d), None if SNR is None else np.asarray(SNR),
            {det: mean[di] for di, det in enumerate(detectors)})


def gen_llf(T_d=50, T_p=4, N=32, n_rx=2, n_tx=2, monte_iter=3, M=4, varn=0.1, seed=0,
            replay=True, varh=1.0, keep=None):
    """Data of PMd/IterationsvsLLF.py:140-149 in its draw order per trial: channelMatrix
    (row-major flatten of h, :16), symbols(T_d), irsMatrix (pilot phases N x T_p DFT over N, :90-92), ones rows inserted into
    the pilot and data phases (:144-145), pilotSymbols, receivedSignals."""
    keep = set(range(monte_iter)) if keep is None else set(keep)
    trials = []
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h = sm.channel_matrix(n_tx, n_rx, N, varh, order="C", rs=rs)
        X_d, _ = sm.symbols(n_tx, M, T_d, rs=rs)
        Ptp, Ptd = sm.irs_matrix(T_p, T_d, N, pilot="dft_n", rs=rs)
        Ptp = sm.insert_direct(Ptp[:N])
        Ptd = sm.insert_direct(Ptd)
        X_p = sm.pilot_symbols(n_tx, M, T_p, rs=rs)
        Y_p, Y_d, U_p, _, h0 = sm.received_signals(T_p, T_d, Ptp, Ptd, n_rx, n_tx, X_d, X_p, h,
                                                   varn, rs=rs)
        if i in keep:
            trials.append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, U_p=U_p, h0=h0, h=h,
                               X_d=np.stack([x.reshape(-1) for x in X_d])))
    return trials


def llf_vs_iteration(T_d=50, T_p=4, N=32, n_rx=2, n_tx=2, itera=5, monte_iter=3, M=4, varn=0.1,
                     seed=0, replay=True, varh=1.0):
    """Mean log-likelihood per EM iteration (PMd/IterationsvsLLF.py:139-154): the exact EM
    (:45-77) with the script's genie LLF (:76: un-squared norms, Z_d from the TRUE data
    symbols), averaged over trials (gen_llf data).  Returns (iterations, mean LLF, mean final
    NMSE)."""
    dist, world, rank = _dist()
    trials = gen_llf(T_d, T_p, N, n_rx, n_tx, monte_iter, M, varn, seed, replay, varh,
                     keep=shard(monte_iter, world, rank).tolist())
    acc = Accumulators(1, n_iters=itera)
    if trials:
        b = _pack(trials, None)
        r = em_batch(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], qam_constellation(M), varn, itera,
                     b["theta0"], mode="soft", x_d_true=np.stack([t["X_d"] for t in trials]))
        acc.add(0, _nmse(r["theta"], b["h"]), llf_values=r["llf"])
    acc.allreduce(dist)
    return np.arange(itera), acc.mean_llf()[0], float(acc.mean_nmse()[0])


def gen_comparison(axis, points, fixed, N=32, n_rx=8, monte_iter=1, M=4, varn=0.1, seed=0,
                   replay=True, varh=1.0, keep=None):
    """Data of the two comparison scripts in their draw orders (n_tx = 1, no direct path).
    axis='td' ("Comparision/Comparision T_d vs NMSE.py":228-242, T_p = fixed): per trial
    channelMatrix1, pilotSymbols(T_p); per point irsMatrix, symbols, received_proposed's noise,
    noise_approx.  axis='tp' ("Comparision/Comparision T_p .py":196-211, T_d = fixed): per trial
    channelMatrix1, symbols(T_d); per point irsMatrix, pilotSymbols, received_proposed,
    noise_approx.  Returns points[k] = list of per-trial dicts holding both legs' inputs."""
    if axis not in ("td", "tp"):
        raise ValueError(axis)
    keep = set(range(monte_iter)) if keep is None else set(keep)
    out = [[] for _ in points]
    if replay:
        np.random.seed(seed)
    for i in range(monte_iter):
        rs = None if replay else _trial_rng(seed, i)
        if not replay and i not in keep:
            continue
        h, F_H, G, h_prop = sm.channel_matrix1(varh, N, n_rx, 1, rs=rs)
        if axis == "td":
            X_p = sm.pilot_symbols(1, M, fixed, rs=rs)
        else:
            X_d, _ = sm.symbols(1, M, fixed, rs=rs)
        for k, pt in enumerate(points):
            tp, td = (fixed, pt) if axis == "td" else (pt, fixed)
            Ptp, Ptd = sm.irs_matrix_nodirect(tp, td, N, rs=rs)
            if axis == "td":
                X_d, _ = sm.symbols(1, M, td, rs=rs)
            else:
                X_p = sm.pilot_symbols(1, M, tp, rs=rs)
            x_p, x_d = np.vstack(X_p), np.vstack(X_d)
            Y_p, Y_d, U_p, _, _ = sm.received_signals(tp, td, Ptp, Ptd, n_rx, 1, X_d, X_p, h_prop,
                                                      varn, rs=rs, with_initial=False)
            z_p, z_d = sm.noise_approx(varn, n_rx, tp, td, rs=rs)
            Y_p_a, Y_d_a = sm.received_approx(h, F_H, Ptp, Ptd, x_d, x_p, z_p, z_d)
            if i in keep:
                out[k].append(dict(Y_d=Y_d, Y_p=Y_p, Psi_d=Ptd, Psi_p=Ptp, U_p=U_p, h=h_prop,
                                   x_p=x_p.reshape(-1), Y_p_a=Y_p_a, Y_d_a=Y_d_a, G=G,
                                   G0=sm.initial_g_approx(Ptp, x_p, Y_p_a)))
    return out


def _comparison(axis, points, fixed, N, n_rx, itera, monte_iter, M, varn, seed, replay, varh):
    dist, world, rank = _dist()
    mine = shard(monte_iter, world, rank).tolist()
    data = gen_comparison(axis, points, fixed, N, n_rx, monte_iter, M, varn, seed, replay, varh,
                          keep=mine)
    cons = qam_constellation(M)
    npt = len(points)
    acc = Accumulators(2 * npt)                       # proposed points, then approximation points
    for k, trials in enumerate(data):
        if not trials:
            continue
        B = len(trials)
        tp = trials[0]["Y_p"].shape[0]
        y_d = np.stack([t["Y_d"] for t in trials])
        y_p = np.stack([t["Y_p"] for t in trials])
        psi_d = np.stack([t["Psi_d"].T for t in trials])
        u_p = np.stack([t["U_p"] for t in trials])
        h = np.stack([t["h"] for t in trials])
        if M == 4:
            # the scripts' per-pilot h_initial (signal_model.initial_estimate_per_pilot): the first
            # E-step's distance sum_p ||y - Z_j theta_p||^2 is, for n_tx = 1 and the constant-modulus
            # 4-QAM, the ordinary one at mean_p theta_p with noise parameter varn / sqrt(T_p)
            th0 = np.stack([sm.initial_estimate_per_pilot(t["U_p"], t["Y_p"], n_rx).mean(axis=0)
                            for t in trials])
            r = em_batch(y_d, y_p, psi_d, u_p, cons, varn / np.sqrt(tp), 1, th0, mode="soft",
                         return_device=itera > 1)
            if itera > 1:
                r = em_batch(y_d, y_p, psi_d, u_p, cons, varn, itera - 1, r["theta"], mode="soft")
        else:
            th0 = np.stack([sm.initial_estimate(t["U_p"], t["Y_p"], n_rx) for t in trials])
            r = em_batch(y_d, y_p, psi_d, u_p, cons, varn, itera, th0, mode="soft")
        acc.add(k, _nmse(r["theta"], h))
        ra = em_approx_batch(np.stack([t["Y_d_a"].T for t in trials]),
                             np.stack([t["Y_p_a"].T for t in trials]), psi_d,
                             np.stack([t["Psi_p"].T for t in trials]),
                             np.stack([t["x_p"] for t in trials]), varn, itera + 1,
                             np.stack([t["G0"] for t in trials]), return_device=True)
        Gt = np.stack([t["G"] for t in trials]).reshape(B, -1)
        acc.add(npt + k, nmse_batch(ra["g"].reshape(B, -1), Gt).cpu().numpy())
    acc.allreduce(dist)
    mean = acc.mean_nmse()
    return np.asarray(points), {"proposed": mean[:npt], "approx": mean[npt:]}


def comparison_vs_td(T_d=(20, 30, 40, 50, 60, 70, 80, 90, 100), T_p=16, N=32, n_rx=8, itera=20,
                     monte_iter=1, M=4, varn=0.1, seed=0, replay=True, varh=1.0):
    """Mean NMSE per data length of the proposed exact EM and of the semi-blind Gaussian
    approximation EM ("Comparision/Comparision T_d vs NMSE.py":203-253; n_tx = 1, no direct
    path).  Returns (T_d, {"proposed": curve, "approx": curve}).

    Approximation leg: G_0 on the host, then ONE sbce_approx_em call per point over every trial
    with itera + 1 updates (`while i <= Iterations`, :114); NMSE = ||G_hat - G||_F^2 / ||G||_F^2
    (:248, trace(abs(E^H E)) / ||G||^2) by sbce_nmse.
    Proposed leg: the exact-soft sbce_em path.  The scripts' h_initial is a per-pilot stack
    (np.linalg.pinv of the LIST Z_p, :181); with M = 4 (constant modulus) and n_tx = 1 that start
    is replayed exactly by two calls -- one iteration at varn / sqrt(T_p) from the mean of the
    per-pilot estimates, then itera - 1 iterations at varn.  For any other M the package's usual
    stacked pseudo-inverse start (signal_model.initial_estimate) is used instead, which is NOT the
    scripts' start."""
    return _comparison("td", tuple(T_d), T_p, N, n_rx, itera, monte_iter, M, varn, seed, replay,
                       varh)


def comparison_vs_tp(T_p=(4, 8, 12, 16, 20, 24, 28, 32, 36, 40), T_d=50, N=32, n_rx=8, itera=15,
                     monte_iter=50, M=4, varn=0.1, seed=0, replay=True, varh=1.0):
    """Mean NMSE per pilot length of the proposed exact EM and of the semi-blind Gaussian
    approximation EM ("Comparision/Comparision T_p .py":171-222); legs, initial values and
    return value as comparison_vs_td."""
    return _comparison("tp", tuple(T_p), T_d, N, n_rx, itera, monte_iter, M, varn, seed, replay,
                       varh)
