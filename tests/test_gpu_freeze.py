"""GPU tier of the fixed-point freeze: once the back substitution of the
batched-panel solve stores the theta it overwrites bit for bit, sbce_em skips the trial's later
iterations.  The outputs must be those of the chain that executes every iteration.

The reference arm needs no switch: ``iters`` chained sbce_em(iters=1) calls, each fed the previous
call's theta, the status words OR-ed.  A one-iteration call can never skip anything (the flags are
re-initialised per call and the flag an iteration sets is read by the next one only).

sbce_em_conv(tol_theta=0, min_iters=1) gives every trial's fixed-point iteration through
iters_done (a trial that stops there has executed iters_done iterations, the last of which
repeated its input), so the tests can assert that trials do freeze -- and that some do not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n_tx, n_rx, P, T_p, T_d, M) and the back substitution the shape ends in
FOLD = (4, 4, 9, 16, 24, 4)      # L = 36 = 32 + 4: backsub4_kernel<4, true> (remainder fold)
EVEN = (4, 2, 10, 16, 24, 4)     # L = 40: backsub4_kernel<2, false>
GEN = (4, 5, 9, 16, 24, 4)       # L = 36, n_rx > 4: backsub_kernel
SHAPES = [FOLD, EVEN, GEN]
SMALL = (2, 2, 8, 16, 24, 4)     # L = 16 <= 64: the one-workgroup M-step (never armed)
B, ITERS = 6, 10
# seeds chosen on the device (see the assertions on sbce_em_conv's iters_done below: they are
# conditions on the inputs; pick another seed if a later change of the arithmetic breaks one)
SEED_HI = {FOLD: 1, EVEN: 1, GEN: 1}                    # 30 dB: at least 3/4 of the trials freeze early
MIXED = {FOLD: (9.0, 1), EVEN: (12.0, 1), GEN: (9.0, 3)}     # (dB, seed): frozen and live trials
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


def _chained(sbce, b, mode, sl=slice(None), iters=ITERS):
    """The unfrozen chain: iters calls of sbce_em(1); computed once per (batch, mode, rows)."""
    key = ("chain", id(b), mode, sl.start, sl.stop, iters)
    if key not in _cache:
        th = b["theta0"][sl]
        status = np.zeros(th.shape[0], dtype=np.int32)
        for _ in range(iters):
            r = sbce.em_batch(*_args(b, sl), 1, th, mode=mode)
            th, status = r["theta"], status | r["status"]
        _cache[key] = (th, status)
    return _cache[key]


def _conv(sbce, b, mode):
    """sbce_em_conv stopping at an exact fixed point: (theta, iters_done)."""
    key = ("conv", id(b), mode)
    if key not in _cache:
        r = sbce.em_batch_conv(*_args(b), ITERS, b["theta0"], tol_theta=0.0, min_iters=1, mode=mode)
        _cache[key] = (r["theta"], r["iters_done"])
    return _cache[key]


def _check_equal(sbce, b, mode):
    """sbce_em(ITERS) against the chain; returns the conv arm's iters_done."""
    res = _plain(sbce, b, mode)
    th, status = _chained(sbce, b, mode)
    assert np.all(np.isfinite(th.view(float)))
    assert np.array_equal(res["theta"], th)
    assert np.array_equal(res["status"], status)
    assert np.array_equal(res["iters_done"], np.full(th.shape[0], ITERS, dtype=np.int32))
    cth, cit = _conv(sbce, b, mode)
    assert np.array_equal(cth, res["theta"])         # an independent path to the same fixed point
    return cit


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_frozen_trials_keep_the_chains_bits(sbce, shape, mode):
    """30 dB: most trials reach their fixed point early and are skipped afterwards; theta, status
    and iters_done are those of the chain that executes every iteration."""
    b = _batch(sbce, shape, 30.0, SEED_HI[shape])
    cit = _check_equal(sbce, b, mode)
    print(f"freeze {_sid(shape)} {mode} 30 dB: fixed point after {cit.tolist()} of {ITERS}")
    assert 4 * np.count_nonzero(cit <= ITERS - 3) >= 3 * B


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_low_snr_chain_is_unchanged(sbce, shape, mode):
    """0 dB: the soft posteriors stay spread and no trial reaches a fixed point -- the armed
    kernels on the never-frozen path; hard decisions may still settle."""
    b = _batch(sbce, shape, 0.0, 3)
    cit = _check_equal(sbce, b, mode)
    print(f"freeze {_sid(shape)} {mode} 0 dB: fixed point after {cit.tolist()} of {ITERS}")
    if mode == "soft":
        assert np.all(cit == ITERS)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_mixed_batch_and_batch_independence(sbce, shape):
    """A batch with frozen and live trials: equal to the chain, and each trial run alone (B = 1)
    has the bits it has inside the batch."""
    snr, seed = MIXED[shape]
    b = _batch(sbce, shape, snr, seed)
    cit = _check_equal(sbce, b, "soft")
    print(f"freeze {_sid(shape)} soft {snr} dB: fixed point after {cit.tolist()} of {ITERS}")
    assert np.any(cit <= ITERS - 2) and np.any(cit == ITERS)
    res = _plain(sbce, b, "soft")
    for i in range(B):
        one = _plain(sbce, b, "soft", slice(i, i + 1))
        assert np.array_equal(one["theta"], res["theta"][i:i + 1]), i
        assert np.array_equal(one["status"], res["status"][i:i + 1]), i


@pytest.mark.parametrize("shape", [FOLD, GEN], ids=_sid)
def test_stale_flags_and_workspace_never_leak(sbce, shape):
    """The flags live in the workspace: a workspace of NaN bit patterns (0xFF bytes: every flag
    set), and the flags a previous run left behind, change nothing."""
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
    """Three stream sub-batches (own workspaces, own flags) against one call, B = 7."""
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


# ------------------------------------------------------------------ paths that are never armed
def test_oracle_stop_is_unchanged(sbce):
    """With h_true the oracle stop owns the flags: a trial stops after iteration it >= 1 (0-based)
    when | ||theta|| - ||h|| | < 1, iters_done counts the executed iterations, and theta is the
    chain's at that iteration.  The stop rule is restated on the host from the chained thetas."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    res = sbce.em_batch(*_args(b), ITERS, b["theta0"], h_true=b["h"])
    th = b["theta0"]
    out = np.zeros_like(th)
    done = np.zeros(B, dtype=bool)
    iters_done = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    nh = np.linalg.norm(b["h"], axis=1)
    for it in range(ITERS):
        r = sbce.em_batch(*_args(b), 1, th, mode="soft")
        th = r["theta"]
        live = ~done
        out[live], iters_done[live] = th[live], it + 1
        status[live] |= r["status"][live]
        gap = np.abs(np.linalg.norm(th, axis=1) - nh)
        assert np.all(np.abs(gap[live] - 1.0) > 1e-6)       # no decision at the threshold
        if it > 0:
            done |= live & (gap < 1.0)
    print(f"oracle stop: iters_done {res['iters_done'].tolist()}")
    assert np.array_equal(res["iters_done"], iters_done)
    assert np.array_equal(res["theta"], out)
    assert np.array_equal(res["status"], status)


def test_noise_chain_is_unchanged(sbce):
    """sbce_em_noise: the state is (theta, sigma^2); the chained calls carry both."""
    b = _batch(sbce, FOLD, 30.0, SEED_HI[FOLD])
    y_d, y_p, psi_d, u_p, cons, varn = _args(b)
    res = sbce.em_batch_noise(y_d, y_p, psi_d, u_p, cons, varn, ITERS, b["theta0"])
    th, v = b["theta0"], np.full(B, varn)
    status = np.zeros(B, dtype=np.int32)
    for _ in range(ITERS):
        r = sbce.em_batch_noise(y_d, y_p, psi_d, u_p, cons, v, 1, th)
        th, v, status = r["theta"], r["varn"], status | r["status"]
    assert np.array_equal(res["theta"], th) and np.array_equal(res["varn"], v)
    assert np.array_equal(res["status"], status)
    assert np.array_equal(res["iters_done"], np.full(B, ITERS, dtype=np.int32))


def test_small_l_chain_is_unchanged(sbce):
    """L <= 64 (n_tx = 2): the one-workgroup M-step, no batched-panel solve, nothing armed."""
    b = _batch(sbce, SMALL, 30.0, 1)
    res = _plain(sbce, b, "soft")
    th, status = _chained(sbce, b, "soft")
    assert np.array_equal(res["theta"], th) and np.array_equal(res["status"], status)
    assert np.array_equal(res["iters_done"], np.full(B, ITERS, dtype=np.int32))
