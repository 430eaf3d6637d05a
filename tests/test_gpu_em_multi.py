"""sbce_em_multi (include/sbce.h): sbce_em on several problems at once, issued iteration by
iteration, a paced problem's launch sequence ending once all its trials are frozen (DESIGN section
3.5).  Every comparison is bit for bit against separate sbce_em calls on fresh copies of the same
inputs: sbce_em issues every iteration and is the yardstick.

Shape unless noted: 4x4, N_RIS 16 (P = 17, L = 68 > 64: the batched-panel solve, so the freeze and
-- n_tx >= 3 -- the moment-repeat rule are armed), T_p 16, T_d 32, 16-QAM.

sbce_em_conv(tol_theta = 0, min_iters = 1) -- code that is not under test -- gives every trial's
stop count c (it executed c iterations, the last of which repeated its input; SBCE_STATUS_CONVERGED
says that it stopped at all).  sbce_em freezes such a trial in iteration c - 1 (0-based), so a
paced problem whose trials all stop has its word set in iteration max c - 1 and the host, which
looks before issuing iteration it >= lead after waiting for iteration it - lead, issues between
max c and max c - 1 + lead iterations (the word is coherent host memory: it may be seen up to
lead - 1 iterations before the event that is waited for).  A problem with a trial that never
stops, an unarmed problem and a capturing stream are issued in full.

Seeds and T_d were chosen on the device so that the preconditions the tests assert first (from the
conv path) hold: 20 dB seed 243, every soft trial stops after 2 or 3 iterations (at most seeds the
soft EM at this shape leaves some trials moving in the last bits for good); 0 dB seed 1, no soft
trial stops within 12; the hard-decision EM settles within 2 iterations at T_d = 32 even at 0 dB,
so its nothing-freezes case runs at T_d = 256, where no trial stops within 12.

Two of the problems the issue lists as unarmed are armed by the condition the library has always
computed: the freeze (the theta compare) does not depend on the E-step, so a pm_soft problem is
paced, and n_tx = 4 takes the batched-panel solve at every L, N_RIS 8 (L = 36) included.  For
those the test asserts what the conv path predicts; the small M-step is covered by a 3x3 shape
(L = 27)."""
import ctypes
import importlib

import numpy as np
import pytest

gpu = pytest.mark.gpu

SHAPE = (4, 4, 16, 16, 32, 16)       # n_tx, n_rx, N_RIS, T_p, T_d, M
ITERS = 12
SEED_HI, SEED_LO = 243, 1            # 20 dB / 0 dB (see the module docstring)
SUBS = (slice(0, 3), slice(3, 5), slice(5, 7))
_cache = {}


def _batch(sbce, snr_db, seed, nb=7, shape=SHAPE, td=None):
    key = ("batch", snr_db, seed, nb, shape, td)
    if key not in _cache:
        n_tx, n_rx, N, T_p, T_d, M = shape
        varn = float(sbce.signal_model.snr_to_varn(snr_db))
        _cache[key] = sbce.signal_model.synthetic_batch(nb, n_tx, n_rx, N, T_p, td or T_d, M, varn,
                                                        seed=seed)
    return _cache[key]


class _Prob:
    """One problem staged on the device from fresh copies of a batch's rows."""

    def __init__(self, sbce, b, rows=slice(None), mode="soft", solve="chol", oracle=False,
                 partition_r=0, ws=None):
        import torch
        em = importlib.import_module(sbce.__name__ + ".em")
        self.mode, self.solve = em._MODES[mode], em._SOLVES[solve]
        self.st = em._Staged(torch, b["y_d"][rows], b["y_p"][rows], b["psi_d"][rows], b["u_p"][rows],
                             b["cons"], b["theta0"][rows], b["varn"], partition_r, solve=self.solve,
                             check="theta0", clone=True)
        st = self.st
        self.xdest = (torch.zeros((st.B, st.T_d, st.n_tx), dtype=torch.complex128, device="cuda")
                      if mode == "hard" else None)
        self.h = em._cdev(torch, b["h"][rows]) if oracle else None
        self.ptrs = st.ptrs(ws=ws, h_true=self.h, x_dest=self.xdest)

    def out(self):
        o = dict(theta=self.st.theta, status=self.st.status, iters_done=self.st.iters_done)
        if self.xdest is not None:
            o["x_dest"] = self.xdest
        return {k: v.cpu().numpy() for k, v in o.items()}


def _call_multi(sbce, probs, iters, lead, streams):
    """The raw call: (rc, iters_issued)."""
    L = sbce._lib
    n = len(probs)
    dims = (ctypes.POINTER(L.Dims) * n)(*[ctypes.pointer(p.st.dims) for p in probs])
    ptrs = (ctypes.POINTER(L.Ptrs) * n)(*[ctypes.pointer(p.ptrs) for p in probs])
    strs = (ctypes.c_void_p * n)(*[s.cuda_stream for s in streams])
    issued = (ctypes.c_int * n)(*([-1] * n))
    rc = L.load().sbce_em_multi(n, dims, ptrs, iters, probs[0].mode, probs[0].solve, strs, lead,
                                issued)
    return rc, list(issued)


def _multi(sbce, probs, iters=ITERS, lead=2, streams=None):
    import torch
    torch.cuda.synchronize()
    streams = streams or [torch.cuda.Stream() for _ in probs]
    rc, issued = _call_multi(sbce, probs, iters, lead, streams)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [p.out() for p in probs], issued


def _single(sbce, b, rows=slice(None), iters=ITERS, **kw):
    """One sbce_em call on fresh copies: the yardstick, computed once per argument set."""
    import torch
    key = ("single", id(b), rows.start, rows.stop, iters, tuple(sorted(kw.items())))
    if key not in _cache:
        p = _Prob(sbce, b, rows, **kw)
        rc = sbce._lib.load().sbce_em(p.st.dims, p.ptrs, iters, p.mode, p.solve,
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        _cache[key] = p.out()
    return _cache[key]


def _conv(sbce, b, mode="soft", iters=ITERS, partition_r=0):
    """(stop counts, stopped) of every trial by sbce_em_conv at an exact fixed point."""
    key = ("conv", id(b), mode, iters, partition_r)
    if key not in _cache:
        r = sbce.em_batch_conv(b["y_d"], b["y_p"], b["psi_d"], b["u_p"], b["cons"], b["varn"], iters,
                               b["theta0"], tol_theta=0.0, min_iters=1, mode=mode,
                               partition_r=partition_r)
        _cache[key] = (r["iters_done"], (r["status"] & sbce._lib.SBCE_STATUS_CONVERGED) != 0)
    return _cache[key]


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _issued_range(cnt, stopped, iters, lead):
    """[lo, hi] of iters_issued for a paced problem (module docstring)."""
    if not stopped.all():
        return iters, iters
    k = int(cnt.max())
    return min(k, iters), min(k - 1 + lead, iters)


# ------------------------------------------------------------------ case 1: early end, 20 dB
@gpu
@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_early_end_keeps_sbce_ems_bits(sbce, mode):
    b = _batch(sbce, 20.0, SEED_HI)
    cnt, stopped = _conv(sbce, b, mode)
    print(f"em_multi 20 dB {mode}: conv stop counts {cnt.tolist()}")
    assert stopped.all() and cnt.max() <= 8                       # the precondition
    outs, issued = _multi(sbce, [_Prob(sbce, b, sl, mode=mode) for sl in SUBS], lead=2)
    print(f"em_multi 20 dB {mode}: iters_issued {issued}")
    whole = _single(sbce, b, mode=mode)
    for sl, o, n in zip(SUBS, outs, issued):
        _same(o, _single(sbce, b, sl, mode=mode))
        _same(o, {k: v[sl] for k, v in whole.items()})            # one 7-trial call, no sub-batches
        assert np.all(o["iters_done"] == ITERS)
        assert cnt[sl].max() <= n < ITERS
        lo, hi = _issued_range(cnt[sl], stopped[sl], ITERS, 2)
        assert lo <= n <= hi


# ------------------------------------------------------------------ case 2: nothing freezes, 0 dB
@gpu
@pytest.mark.parametrize("mode,td", [("soft", 32), ("hard", 256)])
def test_nothing_freezes_issues_everything(sbce, mode, td):
    b = _batch(sbce, 0.0, SEED_LO, td=td)
    cnt, stopped = _conv(sbce, b, mode)
    assert not stopped.any()                                      # the precondition
    outs, issued = _multi(sbce, [_Prob(sbce, b, sl, mode=mode) for sl in SUBS], lead=2)
    assert issued == [ITERS] * 3
    for sl, o in zip(SUBS, outs):
        _same(o, _single(sbce, b, sl, mode=mode))


# ------------------------------------------------------------------ case 3: mixed
@gpu
def test_mixed_problems_with_their_own_dims(sbce):
    hi, lo = _batch(sbce, 20.0, 2, nb=3), _batch(sbce, 0.0, SEED_LO, nb=2)
    (chi, shi), (clo, slo) = _conv(sbce, hi), _conv(sbce, lo)
    assert shi.all() and chi.max() <= 8 and not slo.any()
    outs, issued = _multi(sbce, [_Prob(sbce, hi), _Prob(sbce, lo)], lead=2)
    print(f"em_multi mixed: conv {chi.tolist()} / {clo.tolist()}, iters_issued {issued}")
    assert chi.max() <= issued[0] <= chi.max() + 1 < ITERS and issued[1] == ITERS
    _same(outs[0], _single(sbce, hi))
    _same(outs[1], _single(sbce, lo))


# ------------------------------------------------------------------ case 4: unarmed problems
@gpu
@pytest.mark.parametrize("what", ["oracle", "small", "minnorm"])
def test_unarmed_problems_are_issued_unpaced(sbce, what):
    """h_true set (the oracle stop owns the flags; iters_done compared too, as everywhere), the
    small M-step (3x3, N_RIS 8: L = 27 <= 64, n_tx not in {4, 8}) and the min-norm solve: at
    20 dB, where an armed problem of these inputs ends early, all iterations are issued."""
    shape = (3, 3, 8, 16, 32, 16) if what == "small" else SHAPE
    b = _batch(sbce, 20.0, SEED_HI, shape=shape)
    kw = dict(oracle=True) if what == "oracle" else dict(solve="lstsq") if what == "minnorm" else {}
    outs, issued = _multi(sbce, [_Prob(sbce, b, sl, **kw) for sl in SUBS], lead=2)
    assert issued == [ITERS] * 3
    for sl, o in zip(SUBS, outs):
        _same(o, _single(sbce, b, sl, **kw))


@gpu
@pytest.mark.parametrize("what", ["pm_soft", "nris8"])
def test_problems_armed_without_the_moment_rule(sbce, what):
    """pm_soft (no moment writer carries the fold, but the theta compare is armed whatever the
    E-step) and 4x4 with N_RIS 8 (L = 36: n_tx = 4 takes the batched-panel solve, remainder fold):
    paced problems, equal to sbce_em.  The pm_soft EM at this shape (partition_r = 1, the only list
    size the kernel set has here) never repeats its theta bit for bit -- no trial stops at 20, 30
    or 40 dB at the seeds tried -- so it is the paced path on which nothing ends, and all
    iterations are issued as the issue expects; the N_RIS 8 trials all stop, and their sequences
    end early as the conv path predicts."""
    shape = (4, 4, 8, 16, 32, 16) if what == "nris8" else SHAPE
    kw = dict(mode="pm_soft", partition_r=1) if what == "pm_soft" else {}
    b = _batch(sbce, 20.0, SEED_HI, shape=shape)
    cnt, stopped = _conv(sbce, b, kw.get("mode", "soft"), partition_r=kw.get("partition_r", 0))
    print(f"em_multi {what}: conv {cnt.tolist()} stopped {stopped.tolist()}")
    if what == "pm_soft":
        assert not stopped.any()                                  # the preconditions
    else:
        assert stopped.all() and cnt.max() <= 8
    outs, issued = _multi(sbce, [_Prob(sbce, b, sl, **kw) for sl in SUBS], lead=2)
    print(f"em_multi {what}: iters_issued {issued}")
    for sl, o, n in zip(SUBS, outs, issued):
        _same(o, _single(sbce, b, sl, **kw))
        lo, hi = _issued_range(cnt[sl], stopped[sl], ITERS, 2)
        assert lo <= n <= hi
        assert n == ITERS if what == "pm_soft" else n < ITERS


# ------------------------------------------------------------------ case 5: capture
@gpu
def test_engine_capture_and_replay(sbce):
    import torch
    b = _batch(sbce, 20.0, SEED_HI)
    eng = sbce.EMEngine(b, b["varn"], streams=3)
    assert len(eng.subs) == 3
    eager = eng.run(ITERS).clone()
    torch.cuda.synchronize()
    assert all(n < ITERS for n in eng.iters_issued)               # the eager run is paced
    g = eng.capture(ITERS)
    assert eng.iters_issued == [ITERS] * 3                        # a capturing stream: unpaced
    eng.theta.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.theta, eager)
    assert np.array_equal(eager.cpu().numpy(), _single(sbce, b)["theta"])


@gpu
def test_multi_under_stream_capture(sbce):
    import torch
    b = _batch(sbce, 20.0, SEED_HI)
    probs = [_Prob(sbce, b, sl) for sl in SUBS]
    streams = [torch.cuda.Stream() for _ in probs]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        ev = torch.cuda.Event()
        ev.record(side)
        for st in streams:
            st.wait_event(ev)
        rc, issued = _call_multi(sbce, probs, ITERS, 2, streams)
        for st in streams:
            side.wait_stream(st)
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 0 and issued == [ITERS] * 3
    torch.cuda.synchronize()
    for sl, p in zip(SUBS, probs):                                # a capture executes nothing
        assert torch.equal(p.st.theta, p.st.theta0)
    g.replay()
    torch.cuda.synchronize()
    for sl, p in zip(SUBS, probs):
        _same(p.out(), _single(sbce, b, sl))


# ------------------------------------------------------------------ case 6: reuse
@gpu
def test_back_to_back_calls_on_the_same_streams_and_workspaces(sbce):
    """20 dB, 0 dB, 20 dB on the same streams and workspaces with no synchronise in between: the
    word the first call left set does not end the second, and the third ends early again."""
    import torch
    hi, lo = _batch(sbce, 20.0, SEED_HI), _batch(sbce, 0.0, SEED_LO)
    cnt, stopped = _conv(sbce, hi)
    assert stopped.all() and not _conv(sbce, lo)[1].any()
    first = [_Prob(sbce, hi, sl) for sl in SUBS]
    second = [_Prob(sbce, lo, sl, ws=p.st.ws) for sl, p in zip(SUBS, first)]
    third = [_Prob(sbce, hi, sl, ws=p.st.ws) for sl, p in zip(SUBS, first)]
    streams = [torch.cuda.Stream() for _ in SUBS]
    torch.cuda.synchronize()
    issued = []
    for probs in (first, second, third):
        rc, n = _call_multi(sbce, probs, ITERS, 2, streams)
        assert rc == 0
        issued.append(n)
    torch.cuda.synchronize()
    print(f"em_multi reuse: iters_issued {issued}")
    assert issued[1] == [ITERS] * 3
    for k in (0, 2):
        assert all(cnt[sl].max() <= n < ITERS for sl, n in zip(SUBS, issued[k]))
    for probs, b in ((first, hi), (second, lo), (third, hi)):
        for sl, p in zip(SUBS, probs):
            _same(p.out(), _single(sbce, b, sl))


# ------------------------------------------------------------------ case 7: edges
@gpu
@pytest.mark.parametrize("iters,lead", [(1, 0), (2, 2), (ITERS, 1), (ITERS, ITERS), (ITERS, 0)])
def test_iters_and_lead_edges(sbce, iters, lead):
    """lead = 0 is the library default (2, or iters when smaller): iters = 1 runs with it, since
    lead = 2 > iters = 1 is an argument error (the next test).  lead = iters never looks."""
    b = _batch(sbce, 20.0, SEED_HI)
    cnt, stopped = _conv(sbce, b)
    outs, issued = _multi(sbce, [_Prob(sbce, b, sl) for sl in SUBS], iters=iters, lead=lead)
    eff = lead or min(2, iters)
    for sl, o, n in zip(SUBS, outs, issued):
        _same(o, _single(sbce, b, sl, iters=iters))
        lo, hi = _issued_range(cnt[sl], stopped[sl], iters, eff)
        if eff >= iters:
            lo = hi = iters
        assert lo <= n <= hi, (n, lo, hi)


@gpu
def test_lead_past_iters_is_refused_and_touches_nothing(sbce):
    import torch
    b = _batch(sbce, 20.0, SEED_HI)
    probs = [_Prob(sbce, b, sl) for sl in SUBS]
    streams = [torch.cuda.Stream() for _ in probs]
    assert _call_multi(sbce, probs, 1, 2, streams)[0] == -1
    bad = sbce._lib.Ptrs.from_buffer_copy(probs[1].ptrs)
    bad.theta = None
    probs[1].ptrs = bad
    assert _call_multi(sbce, probs, ITERS, 2, streams)[0] == -1
    torch.cuda.synchronize()
    for p in probs:                                               # nothing was issued for any
        assert torch.equal(p.st.theta, p.st.theta0)


@gpu
@pytest.mark.parametrize("nb", [1, 7])
def test_one_problem(sbce, nb):
    """n = 1, with B = 1 and B = 7."""
    b = _batch(sbce, 20.0, SEED_LO if nb == 1 else SEED_HI, nb=nb)
    cnt, stopped = _conv(sbce, b)
    assert stopped.all()
    outs, issued = _multi(sbce, [_Prob(sbce, b)], lead=2)
    _same(outs[0], _single(sbce, b))
    assert cnt.max() <= issued[0] <= cnt.max() + 1 < ITERS


# ------------------------------------------------------------------ case 8: validation, CPU tier
def test_validation_without_gpu(sbce):
    """Every argument of every problem is checked before any HIP call: the pointers here are
    made-up addresses, so a call that got past its checks would not return an argument error."""
    L = sbce._lib
    lib = L.load()
    d = L.Dims(3, 4, 4, 17, 16, 32, 16, 0, 0.1)
    good = L.Ptrs(y_d=256, y_p=256, psi_d=256, u_p=256, cons=256, theta=256, status=256,
                  workspace=256, workspace_bytes=1 << 62)
    null_theta = L.Ptrs.from_buffer_copy(good)
    null_theta.theta = None
    huge = L.Dims(2, 8, 4, 1025, 16, 64, 16, 1, 0.1)              # L = 8200 > 8192: unsupported

    def call(n, dims, ptrs, iters=12, lead=2, mode=L.SBCE_ESTEP_SOFT, arrays=(True, True, True)):
        k = max(len(dims), 1)
        da = (ctypes.POINTER(L.Dims) * k)(*[ctypes.pointer(x) for x in dims])
        pa = (ctypes.POINTER(L.Ptrs) * k)(*[ctypes.pointer(x) for x in ptrs])
        sa = (ctypes.c_void_p * k)()
        issued = (ctypes.c_int * k)(*([-7] * k))
        rc = lib.sbce_em_multi(n, da if arrays[0] else None, pa if arrays[1] else None, iters, mode,
                               L.SBCE_SOLVE_CHOL, sa if arrays[2] else None, lead, issued)
        assert list(issued) == [-7] * k                           # an error reports nothing
        return rc

    three = ([d] * 3, [good] * 3)
    assert call(0, *three) == -1
    assert call(9, [d] * 9, [good] * 9) == -1
    for k in range(3):
        assert call(3, *three, arrays=tuple(i != k for i in range(3))) == -1
    assert call(3, *three, lead=-1) == -1
    assert call(3, *three, iters=4, lead=5) == -1
    assert call(3, [d] * 3, [good, good, null_theta]) == -1
    assert call(3, [d] * 3, [good, null_theta, good]) == -1
    assert call(3, [d, d, huge], [good] * 3, mode=L.SBCE_ESTEP_PM_SOFT) == -2
    assert call(3, [huge, d, d], [good] * 3, mode=L.SBCE_ESTEP_PM_SOFT) == -2
