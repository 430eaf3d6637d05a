"""GPU tier of the moment-repeat rule: the E-step's moment stores compare the
word they overwrite, and a trial whose moments repeat bit for bit skips its M-step -- the back
substitution freezes it instead, one M-step before the theta compare of the fixed-point freeze
would.  theta, status and iters_done must be those of the chain that executes every iteration.

The reference arm is test_gpu_freeze.py's: ``iters`` chained sbce_em(iters=1) calls.  A
one-iteration call compares nothing (iteration 0 of a call never does) and can skip nothing.

The A/B build counts the trial-M-steps the rule skipped (sbce_debug_momskip); the product build
has no counter.  The seeds are conditions on the inputs, as in test_gpu_freeze.py: pick another
seed if a later change of the arithmetic breaks one."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n_tx, n_rx, P, T_p, T_d, M) and the back substitution the shape ends in
FOLD = (4, 4, 9, 16, 24, 4)      # L = 36 = 32 + 4: backsub4_kernel<4, true> (remainder fold)
EVEN = (4, 2, 10, 16, 24, 4)     # L = 40: backsub4_kernel<2, false>
GEN = (4, 5, 9, 16, 24, 4)       # L = 36, n_rx > 4: backsub_kernel
SHAPES = [FOLD, EVEN, GEN]
# L = 69 > 64 at n_tx = 3, 16-QAM: the batched-panel solve with the tree pass, the enumeration
# <3, *>, the bounds pass and the listed sweep <3, 3, *, 1> as the folded moment writers.  In
# test_skipped_msteps_keep_the_chains_bits in hard mode only: no seed 1..40 meets its soft
# condition (see test_nt3_equals_the_chain for what they gave at 30 dB).
NT3 = (3, 3, 23, 16, 24, 16)
SMALL = (2, 2, 8, 16, 24, 4)     # L = 16 <= 64: the one-workgroup M-step (never armed)
NT2 = (2, 2, 40, 96, 24, 16)     # L = 80: the theta freeze is armed, the n_tx = 2 E-step passes
                                 # carry no fold -- the rule stays unarmed
B, ITERS = 6, 10
# 30 dB: at least 3/4 of the trials reach their fixed point before the last iteration, and the
# moments announce every one of them.  Chosen on the device: with test_gpu_freeze.py's seed 1 the
# soft E-step of FOLD rewrites 2 of the 6 trials' moments equal in value but not in the sign of a
# zero (a symbol resolved by the sweep at iteration 0 and by the tree pass or the enumeration at
# iteration 1: -0 against +0 in a lower-triangle entry of S_t) -- bit for bit they changed, and
# the theta compare freezes those trials one M-step later.  EVEN (n_rx < n_tx: the sweep is the
# only writer) met the soft condition for none of the seeds 1..12 and for 13, 22, 29, 33, 41.
SEED_HI = {FOLD: 7, EVEN: 29, GEN: 7, NT3: 7}
# (dB, seed): frozen and live trials.  NT3, chosen on the device: below 15 dB no trial of the
# seeds 1..6 stops early; at 15 dB seed 1 stops after [10, 4, 3, 4, 10, 4] iterations.
MIXED = {FOLD: (9.0, 1), EVEN: (12.0, 1), GEN: (9.0, 3), NT3: (15.0, 1)}
_cache = {}


def _sid(s):
    return "x".join(map(str, s))


def _batch(sbce, shape, snr_db, seed, nb=B):
    key = ("batch", shape, snr_db, seed, nb)
    if key not in _cache:
        n_tx, n_rx, P, T_p, T_d, M = shape
        varn = float(sbce.signal_model.snr_to_varn(snr_db))
        _cache[key] = sbce.signal_model.synthetic_batch(nb, n_tx, n_rx, P - 1, T_p, T_d, M, varn,
                                                        seed=seed)
    return _cache[key]


def _args(b, sl=slice(None)):
    return b["y_d"][sl], b["y_p"][sl], b["psi_d"][sl], b["u_p"][sl], b["cons"], b["varn"]


def _plain(sbce, b, mode, sl=slice(None), iters=ITERS):
    """One sbce_em(iters) call: the arm under test."""
    return sbce.em_batch(*_args(b, sl), iters, b["theta0"][sl], mode=mode)


def _chain(sbce, b, mode, sl=slice(None), iters=ITERS):
    """The chain that skips nothing: iters calls of sbce_em(1).  Returns every iterate
    (iters + 1, rows, K) and the OR of the status words."""
    th = b["theta0"][sl]
    out = [th]
    status = np.zeros(th.shape[0], dtype=np.int32)
    for _ in range(iters):
        r = sbce.em_batch(*_args(b, sl), 1, th, mode=mode)
        th, status = r["theta"], status | r["status"]
        out.append(th)
    return np.stack(out), status


def _chained(sbce, b, mode, sl=slice(None)):
    """_chain on the product library, computed once per (batch, mode, rows): (theta, status)."""
    key = ("chain", id(b), mode, sl.start, sl.stop)
    if key not in _cache:
        ths, status = _chain(sbce, b, mode, sl)
        _cache[key] = (ths, status)
    ths, status = _cache[key]
    return ths[-1], status


def _conv(sbce, b, mode):
    """sbce_em_conv stopping at an exact fixed point: (theta, iters_done)."""
    key = ("conv", id(b), mode)
    if key not in _cache:
        r = sbce.em_batch_conv(*_args(b), ITERS, b["theta0"], tol_theta=0.0, min_iters=1, mode=mode)
        _cache[key] = (r["theta"], r["iters_done"])
    return _cache[key]


def _reset(lib):
    assert lib.sbce_debug_momskip(None, 1) == 0


def _skipped(lib):
    n = ctypes.c_ulonglong(0)
    assert lib.sbce_debug_momskip(ctypes.byref(n), 0) == 0
    return int(n.value)


def _assert_run(res, th, status):
    assert np.array_equal(res["theta"], th)
    assert np.array_equal(res["status"], status)
    assert np.array_equal(res["iters_done"], np.full(th.shape[0], ITERS, dtype=np.int32))


_SKIPPED = [(s, m) for s in SHAPES for m in ("soft", "hard")] + [(NT3, "hard")]


@pytest.mark.parametrize("shape,mode", _SKIPPED, ids=[f"{_sid(s)}-{m}" for s, m in _SKIPPED])
def test_skipped_msteps_keep_the_chains_bits(sbce, shape, mode):
    """30 dB: most trials' moments repeat early.  Product and A/B build equal the chain and the
    conv arm's fixed point; the A/B build skipped at least one M-step per trial that the conv arm
    stopped before the last iteration."""
    b = _batch(sbce, shape, 30.0, SEED_HI[shape])
    th, status = _chained(sbce, b, mode)
    assert np.all(np.isfinite(th.view(float)))
    _assert_run(_plain(sbce, b, mode), th, status)
    cth, cit = _conv(sbce, b, mode)
    assert np.array_equal(cth, th)
    early = int(np.count_nonzero(cit < ITERS))
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        _assert_run(_plain(sbce, b, mode), th, status)
        n = _skipped(lib)
    print(f"momfreeze {_sid(shape)} {mode} 30 dB: fixed point after {cit.tolist()} of {ITERS}, "
          f"{n} M-steps skipped")
    assert 4 * early >= 3 * B
    assert n >= early


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_nt3_equals_the_chain(sbce, mode):
    """NT3 at 30 dB: theta, status and iters_done of the product and the A/B build are the
    chain's, and the conv arm stops at the same theta.  Seen on the device for every seed 1..40:
    T_p + T_d = 40 < L = 69 and the posteriors are one-hot, so R is rank deficient (every trial
    carries SBCE_STATUS_NONHPD, the dropped-pivot solve), the second iteration reproduces the
    first one's theta bit for bit in all six trials, and the theta compare freezes them there.
    Hard: the decisions of iteration 1 repeat iteration 0's and the rule skips 6 M-steps (one a
    trial).  Soft: the moments at theta_0 and theta_1 differ, the rule skips nothing (seed 33: 1)
    before the freeze -- no seed meets `skipped >= early` of
    test_skipped_msteps_keep_the_chains_bits in soft mode, so NT3 is in that test in hard mode
    only.  Its other conditions are asserted here for both modes."""
    b = _batch(sbce, NT3, 30.0, SEED_HI[NT3])
    th, status = _chained(sbce, b, mode)
    assert np.all(np.isfinite(th.view(float)))
    _assert_run(_plain(sbce, b, mode), th, status)
    cth, cit = _conv(sbce, b, mode)
    assert np.array_equal(cth, th)
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        _assert_run(_plain(sbce, b, mode), th, status)
        n = _skipped(lib)
    print(f"momfreeze {_sid(NT3)} {mode} 30 dB: fixed point after {cit.tolist()} of {ITERS}, "
          f"{n} M-steps skipped, status {status.tolist()}")
    # the seed-dependent conditions of test_skipped_msteps_keep_the_chains_bits, all but soft
    # mode's `n >= early`: the fold is armed at n_tx = 3 and the <3, *> writers announce a repeat
    early = int(np.count_nonzero(cit < ITERS))
    assert 4 * early >= 3 * B
    if mode == "hard":
        assert n >= early


@pytest.mark.parametrize("shape", SHAPES + [NT3], ids=_sid)
def test_low_snr_soft_skips_nothing(sbce, shape):
    """0 dB, soft: the posteriors stay spread, no trial's moments repeat -- the folded stores on
    the path that never skips."""
    b = _batch(sbce, shape, 0.0, 3)
    th, status = _chained(sbce, b, "soft")
    _assert_run(_plain(sbce, b, "soft"), th, status)
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        _assert_run(_plain(sbce, b, "soft"), th, status)
        assert _skipped(lib) == 0


@pytest.mark.parametrize("shape", SHAPES + [NT3], ids=_sid)
def test_mixed_batch_and_batch_independence(sbce, shape):
    """A batch with skipped and live trials: equal to the chain, and each trial run alone (B = 1)
    has the bits it has inside the batch."""
    snr, seed = MIXED[shape]
    b = _batch(sbce, shape, snr, seed)
    th, status = _chained(sbce, b, "soft")
    res = _plain(sbce, b, "soft")
    _assert_run(res, th, status)
    cit = _conv(sbce, b, "soft")[1]
    assert np.any(cit <= ITERS - 2) and np.any(cit == ITERS)
    for i in range(B):
        one = _plain(sbce, b, "soft", slice(i, i + 1))
        assert np.array_equal(one["theta"], res["theta"][i:i + 1]), i
        assert np.array_equal(one["status"], res["status"][i:i + 1]), i


@pytest.mark.parametrize("shape", [FOLD, GEN, NT3], ids=_sid)
def test_stale_workspace_never_leaks(sbce, shape):
    """The change words and the moments live in the workspace: a workspace of 0xFF bytes (every
    word set, NaN moments), and what a previous run left behind, change nothing -- iteration 0
    compares nothing and the words are zeroed per call."""
    import torch
    b = _batch(sbce, shape, 30.0, SEED_HI[shape])
    th, status = _chained(sbce, b, "soft")
    eng = sbce.EMEngine(b, b["varn"])
    eng.ws_all.fill_(0xFF)
    for _ in range(2):
        out = eng.run(ITERS).clone()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), th)
        assert np.array_equal(eng.status.cpu().numpy(), status)


def test_stream_sub_batches(sbce):
    """Three stream sub-batches (own workspaces, own change words) against one call, B = 7."""
    import torch
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD], nb=7)
    out = []
    for k in (1, 3):
        eng = sbce.EMEngine(b, b["varn"], streams=k)
        assert len(eng.subs) == (3 if k == 3 else 0)
        th = eng.run(ITERS).clone()
        torch.cuda.synchronize()
        out.append((th.cpu().numpy(), eng.status.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][0], _chained(sbce, b, "soft")[0])


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_sphere_pass_off(sbce, mode):
    """SBCE_ESTEP_SPHERE=0 (A/B build): the unlisted MFMA sweep is the only moment writer.  The
    run equals the chain of the same build and switch, and M-steps are skipped."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    with sbce._lib.debug_env(SBCE_ESTEP_SPHERE="0") as lib:
        ths, status = _chain(sbce, b, mode)
        _reset(lib)
        _assert_run(_plain(sbce, b, mode), ths[-1], status)
        n = _skipped(lib)
    assert np.all(status & sbce._lib.SBCE_STATUS_DEBUG)
    print(f"momfreeze sphere off {mode}: {n} M-steps skipped")
    assert n > 0


# ------------------------------------------------------------------ paths that are never armed
def test_oracle_stop_is_unchanged(sbce):
    """With h_true the oracle stop owns the flags: theta is the chain's at the iteration the
    stop rule (restated on the host) ends the trial, and no M-step is skipped."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    ths, _ = _chain(sbce, b, "soft")
    nh = np.linalg.norm(b["h"], axis=1)
    iters_done = np.full(B, ITERS, dtype=np.int32)
    for i in range(B):
        for it in range(1, ITERS):
            if abs(np.linalg.norm(ths[it + 1, i]) - nh[i]) < 1.0:
                iters_done[i] = it + 1
                break
    out = ths[iters_done, np.arange(B)]
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        res = sbce.em_batch(*_args(b), ITERS, b["theta0"], h_true=b["h"])
        assert _skipped(lib) == 0
    assert np.array_equal(res["iters_done"], iters_done)
    assert np.array_equal(res["theta"], out)


def test_noise_chain_is_unchanged(sbce):
    """sbce_em_noise: the state is (theta, sigma^2); the chained calls carry both."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    y_d, y_p, psi_d, u_p, cons, varn = _args(b)
    th, v = b["theta0"], np.full(B, varn)
    status = np.zeros(B, dtype=np.int32)
    for _ in range(ITERS):
        r = sbce.em_batch_noise(y_d, y_p, psi_d, u_p, cons, v, 1, th)
        th, v, status = r["theta"], r["varn"], status | r["status"]
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        res = sbce.em_batch_noise(y_d, y_p, psi_d, u_p, cons, varn, ITERS, b["theta0"])
        assert _skipped(lib) == 0
    assert np.array_equal(res["theta"], th) and np.array_equal(res["varn"], v)
    assert np.array_equal(res["status"], status)
    assert np.array_equal(res["iters_done"], np.full(B, ITERS, dtype=np.int32))


def test_conv_chain_is_unchanged(sbce):
    """sbce_em_conv owns the flags: every trial's theta is the chain's at the iteration the conv
    stop ended it, and no M-step is skipped."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    ths, _ = _chain(sbce, b, "soft")
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        r = sbce.em_batch_conv(*_args(b), ITERS, b["theta0"], tol_theta=0.0, min_iters=1)
        assert _skipped(lib) == 0
    cit = r["iters_done"]
    assert np.all((cit >= 1) & (cit <= ITERS))
    assert np.array_equal(r["theta"], ths[cit, np.arange(B)])
    # the stop is the first iteration that reproduced its input
    for i in range(B):
        same = [k for k in range(1, ITERS + 1) if np.array_equal(ths[k, i], ths[k - 1, i])]
        assert cit[i] == (same[0] if same else ITERS), i


@pytest.mark.parametrize("shape", [SMALL, NT2], ids=_sid)
def test_unarmed_shapes_are_unchanged(sbce, shape):
    """n_tx = 2: the one-workgroup M-step at L <= 64 (nothing armed), and the batched-panel solve
    at L = 80, where the theta freeze is armed and the E-step's factorised passes carry no fold."""
    b = _batch(sbce, shape, 30.0, 1)
    th, status = _chained(sbce, b, "soft")
    _assert_run(_plain(sbce, b, "soft"), th, status)
    with sbce._lib.debug_env() as lib:
        _reset(lib)
        _assert_run(_plain(sbce, b, "soft"), th, status)
        assert _skipped(lib) == 0
