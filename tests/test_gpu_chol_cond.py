"""GPU tier: the M-step's Hermitian solve R X = B^H on ill-conditioned HPD systems (cond 1e4 ...
1e10) and on systems with pivots planted on either side of the drop threshold -- every route
launch_mstep_small, launch_chol_batched and launch_chol_large select, and their A/B arms.

Everything goes through sbce.mstep_batch.  The reference is tests/solve_ref.chol_solve_ld (an
unblocked long-double Cholesky under the device's pivot rule) of the R and B^H THE DEVICE
RETURNED: that isolates the solve (the builds have tests/test_gpu_mstep_build.py); the device's R
is held to the oracle's at 1e-12 on the lower triangle besides.  tests/test_solve_ref.py shows on
the CPU that the float64 restatement of the solve meets every bar below on these inputs with
room to spare (forward error <= 0.09 eps cond, backward error <= 0.14 eps).

Bars (none measured on the code under test):
  forward   rel(theta_dev, theta_ref) <= max(1e-12, 1e-15 cond_2(R_dev)), the constants of
            test_gpu_em.py's solve checks; ten times that on the arms that form complex products
            from three real MFMAs (the Gauss trick, SBCE_CPLX3: the batched and large routes
            under SBCE_SOLVE_CHOL);
  backward  eta_dev <= 8 max(eta_cpu, eps), eta = ||R X - B^H||_F / (||R||_F ||X||_F) and eta_cpu
            the float64 restatement's on the same R, B^H: independent of cond, it is what
            catches a solve that is only roughly right.  8: blocked and MFMA summation orders
            differ from the unblocked one, and the Gauss product raises the constant a little;
  status    nothing but SBCE_STATUS_DEBUG where the reference's smallest pivot is >= 1e3 tol.

Every case prints cond, err / (eps cond) and eta_dev / eta_cpu; run with -s to read them.
DESIGN.md section 3.5g records the worst per route as measured on the MI355X, and the two fixes
the planted-pivot test forced (CHOL_DROP on CHOL's route; +0 for a dropped unknown in the
one-workgroup kernels).
"""
import functools
import hashlib

import numpy as np
import pytest

import solve_ref as sr
from conftest import rel

pytestmark = pytest.mark.gpu

ARMS = {
    "small": [{}, dict(SBCE_MSTEP_SMALL="0"), dict(SBCE_MSTEP_SMALL="1"),
              dict(SBCE_MSTEP_SMALL="v"), dict(SBCE_SMALL_SOLVE="col")],
    "batched": [{}, dict(SBCE_CPLX3="0"), dict(SBCE_CHOL_IMPL="valu"), dict(SBCE_BACKSUB="1")],
    "large": [{}],
}


def arm_name(env):
    return ",".join(f"{k}={v}" for k, v in env.items()) or "default"


def three_mfma(shape, env):
    """The arm's complex products come from three real MFMAs: the batched panel factorisation
    (also what SBCE_MSTEP_SMALL=0 sends a small shape to) and the large route, unless
    SBCE_CPLX3=0 or the VALU Cholesky is asked for.  The one-workgroup kernels use four."""
    if env.get("SBCE_CPLX3") == "0" or env.get("SBCE_CHOL_IMPL") == "valu":
        return False
    return sr.family(shape) != "small" or env.get("SBCE_MSTEP_SMALL") == "0"


def run(sbce, inp, env=None, nb=None, **kw):
    args = sr.args_of(inp)
    if nb is not None:
        args = tuple(a[:nb] if np.ndim(a) > 1 else a for a in args[:-1]) + args[-1:]
    try:
        if not env:
            return sbce.mstep_batch(*args, **kw)
        with sbce._lib.debug_env(**env):
            return sbce.mstep_batch(*args, **kw)
    except sbce._lib.SbceError as e:
        raise AssertionError(f"{arm_name(env or {})}: {e}") from e


# ------------------------------------------------------------------ shared references: read only
@functools.lru_cache(maxsize=None)
def graded(sbce, shape, decades):
    """The inputs of (shape, decades) and the oracle's R per trial, computed once."""
    inp = sr.graded_inputs(sbce, *shape, decades, sr.SEED, sr.trials_of(shape))
    return inp, [sr.host_system(inp, i)[0] for i in range(sr.trials_of(shape))]


_REF = {}


def reference(shape, decades, i, R, rhs):
    """solve_ref.reference of the system the device returned, once per (shape, decades, trial)
    and content: the arms of a route that share the build kernels return the same bits."""
    key = (shape, decades, i, hashlib.sha1(R.tobytes() + rhs.tobytes()).hexdigest())
    if key not in _REF:
        _REF[key] = sr.reference(R, rhs, shape[1])
    return _REF[key]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ------------------------------------------------------------------ a. graded spectrum
GRADED = [pytest.param(shape, decades, env, id=f"{shape}-{decades}-{arm_name(env)}".replace(" ", ""))
          for shape in sr.SHAPES for decades in sr.decades_of(shape)
          for env in ARMS[sr.family(shape)]]


@pytest.mark.parametrize("shape,decades,env", GRADED)
def test_graded_spectrum_forward_and_backward_error(sbce, shape, decades, env):
    """R with the spectrum logspace(0, -decades, P) x (1 ... 1 + |v|^2 / 2), dense, two trials
    (one above L = 512): no flag, theta finite, forward and backward error under the module's
    bars.

    Measured on the MI355X, worst over shapes, decades and trials:
      route, arm                                    err/(eps cond)  eta_dev/eps  eta_dev/eta_cpu
      small, 4-column-panel solve (default)              0.056         0.18           1.6
      small, SBCE_SMALL_SOLVE=col                        0.055         0.15           1.7
      small, mstep_small_kernel (default, =1, =v)        0.057         0.23           2.0
      small shapes, SBCE_MSTEP_SMALL=0 (batched path)    0.107         0.44           5.1
      batched, backsub4 (default)                        0.128         0.26           5.5
      batched, general back substitution                 0.128         0.26           5.1
      batched, SBCE_CPLX3=0                              0.070         0.22           3.7
      batched, SBCE_CHOL_IMPL=valu                       0.073         0.22           2.8
      large                                              0.104         0.14           2.7
    against bars of 4.5 (45 on the three-MFMA arms) and 8 (eta_cpu < eps everywhere)."""
    n_tx, n_rx, N = shape
    inp, R_host = graded(sbce, shape, decades)
    th, R, rhs, st = run(sbce, inp, env, solve="chol")
    L = inp["L"]
    assert R.shape[1] == L == (N + 1) * n_tx
    assert not (st & sbce._lib.SBCE_STATUS_PILOT).any()
    assert not (st & ~sbce._lib.SBCE_STATUS_DEBUG).any(), st
    assert np.isfinite(th).all()
    lo = np.tril_indices(L)
    for i in range(sr.trials_of(shape)):
        assert rel(R[i][lo], R_host[i][lo]) < 1e-12
        ref = reference(shape, decades, i, R[i], rhs[i])
        assert not ref["dropped"].any() and float(ref["piv"].min()) >= 1e3 * ref["tol"]
        err = sr.rel_ld(th[i], ref["theta"])
        eta = sr.backward_error(R[i], th[i], rhs[i], n_rx)
        bar = sr.forward_bar(ref["cond"], three_mfma(shape, env))
        print(f"[chol-cond] {sr.family(shape)} {shape} L={L} decades {decades} "
              f"{arm_name(env)} trial {i}: cond {ref['cond']:.2e} err {err:.2e} "
              f"err/(eps cond) {err / (sr.EPS * ref['cond']):.4f} eta_dev/eps {eta / sr.EPS:.3f} "
              f"eta_dev/eta_cpu {eta / ref['eta_cpu']:.2f} bar/err {bar / max(err, 1e-300):.1f}")
        assert err <= bar, (err, bar)
        assert eta <= 8 * max(ref["eta_cpu"], sr.EPS), (eta, ref["eta_cpu"])


# ------------------------------------------------------------------ b. planted pivots
def cross_arm(shape):
    """One cross-check arm per family: the column-at-a-time solve where the 4-column-panel one
    runs (n_tx <= 2, P <= 16, n_rx <= 4), the VALU one-workgroup kernel at the other small
    shapes, four real MFMAs per complex product on the batched and large routes."""
    n_tx, n_rx, N = shape
    if sr.family(shape) != "small":
        return dict(SBCE_CPLX3="0")
    if n_tx <= 2 and N + 1 <= 16 and n_rx <= 4:
        return dict(SBCE_SMALL_SOLVE="col")
    return dict(SBCE_MSTEP_SMALL="v")


PLANTED = [pytest.param(shape, big, name, blk, id=f"{shape}-{big}-{name}".replace(" ", ""))
           for shape in sr.SHAPES for big in ("first", "last")
           for name, blk in sr.tiny_positions(shape).items()]


def check_planted(sbce, shape, blk, out, what):
    """Status, the dropped block's zeros and every other block against its own long-double
    solve.  Returns the bits of the CPU restatement's theta on the dropped block."""
    from oracle.em_reduced import mstep_chol_policy
    n_tx, n_rx, N = shape
    th, R, rhs, st = out
    P, L = N + 1, (N + 1) * n_tx
    mask = sr.planted_mask(shape, blk)
    nonhpd = sbce._lib.SBCE_STATUS_NONHPD
    assert not (st & sbce._lib.SBCE_STATUS_PILOT).any(), what
    assert (int(st[0]) & ~sbce._lib.SBCE_STATUS_DEBUG) == nonhpd, (what, st)
    assert (int(st[1]) & ~sbce._lib.SBCE_STATUS_DEBUG) == 0, (what, st)
    assert np.isfinite(th).all(), what
    blocks = np.kron(np.eye(P), np.ones((n_tx, n_tx))) > 0
    for i in range(2):
        assert np.abs(R[i][~blocks]).max(initial=0.0) <= 1e-40 * sr.S_TINY, what
        want = mask if i == 0 else np.zeros_like(mask)
        R64 = sr.herm_lower(R[i], np.complex128)
        if sr.family(shape) != "large":
            th_cpu, bad = mstep_chol_policy(R64, rhs[i])
        else:
            # above L = 512 the whole-R restatement costs seconds: block by block under the
            # whole R's tol, which for a block-diagonal R is the same arithmetic
            tol = sr.REL_TOL * R64.diagonal().real.max()
            th_cpu, bad = np.zeros(L * n_rx, dtype=complex), np.zeros(L, dtype=bool)
            for t in range(P):
                sl = slice(t * n_tx, (t + 1) * n_tx)
                Rt = R64[sl, sl]
                th_t, bad[sl] = mstep_chol_policy(Rt, rhs[i][sl],
                                                  rel_tol=tol / Rt.diagonal().real.max())
                th_cpu[t * n_tx * n_rx:(t + 1) * n_tx * n_rx] = th_t
        assert np.array_equal(bad, want), (what, i)
        X = th[i].reshape(L, n_rx)
        Xc = th_cpu.reshape(L, n_rx)
        # the dropped unknowns are zero to the bit, signs included, as the restatement's are
        assert np.array_equal(bits(X[want]), bits(Xc[want])), (what, i, X[want])
        assert not (bits(X[want]) & np.uint64(0x7FFFFFFFFFFFFFFF)).any(), (what, i)
        worst = 0.0
        for t in range(P):
            if i == 0 and t == blk:
                continue
            sl = slice(t * n_tx, (t + 1) * n_tx)
            Rt = R[i][sl, sl]
            ref, dropped, _ = sr.chol_solve_ld(Rt, rhs[i][sl])
            assert not dropped.any()
            cond = float(np.linalg.cond(sr.herm_lower(Rt, np.complex128)))
            err = sr.rel_ld(X[sl], ref)
            worst = max(worst, err / sr.forward_bar(cond))
            assert err <= sr.forward_bar(cond), (what, i, t, err, cond)
        print(f"[chol-cond] planted {shape} {what} trial {i}: worst block err/bar {worst:.4f}")


@pytest.mark.parametrize("shape,big,name,blk", PLANTED)
def test_planted_pivots_are_dropped_exactly_where_planted(sbce, shape, big, name, blk):
    """R block diagonal (psi_t = e_t) with the n_tx x n_tx blocks S_t: one block at scale 1 sets
    tol = 1e-14 max diag R, one at 1e-17 has every pivot >= 100 times below tol, the others at
    1e-11 are >= 100 times above; trial 1 of the same call has no tiny block.  With big = "last"
    the largest diagonal entry lies in the last partial tile (the folded remainder at L = 36,
    68, 260): a tol taken over a short extent would keep the tiny block.

    Trial 0 is flagged NONHPD and trial 1 is not; the tiny block's unknowns are zero to the bit
    (as the CPU restatement's), every other block equals its own long-double solve at
    max(1e-12, 1e-15 cond(S_t)); solve="drop" gives bitwise solve="chol"'s theta and status;
    both are bitwise the same in a 0x00 and a 0xFF workspace; one cross-check arm per family
    meets the same."""
    n_tx, n_rx, N = shape
    s, big_block = sr.planted_scales(shape, big, blk)
    inp = sr.planted_inputs(sbce, n_tx, n_rx, N, s, sr.SEED)
    L = inp["L"]
    lo = np.tril_indices(L)
    outs = {}
    for solve in ("chol", "drop"):
        for fill in (0x00, 0xFF):
            outs[solve, fill] = run(sbce, inp, solve=solve, ws_fill=fill)
    th0, R0, rhs0, st0 = outs["chol", 0x00]
    for i in range(2):
        assert rel(R0[i][lo], sr.host_system(inp, i)[0][lo]) < 1e-12
        assert int(np.argmax(R0[i].diagonal().real)) // n_tx == big_block
    check_planted(sbce, shape, blk, outs["chol", 0x00], f"big {big} tiny {name} chol")
    for key, out in outs.items():
        assert np.array_equal(bits(out[0]), bits(th0)), key
        assert np.array_equal(out[3], st0), key
    env = cross_arm(shape)
    check_planted(sbce, shape, blk, run(sbce, inp, env, solve="chol"),
                  f"big {big} tiny {name} {arm_name(env)}")


# ------------------------------------------------------------------ c. batch / workspace independence
@pytest.mark.parametrize("shape", [(2, 2, 15), (4, 1, 16), (4, 4, 28), (4, 4, 149)])
def test_ill_conditioned_solve_is_batch_and_workspace_independent(sbce, shape):
    """decades = 10, one shape per family: trial 0's theta and status are bitwise the same solved
    alone, in a batch of 3, in a batch of 65, in a repeated call, and in a 0x00 and a 0xFF
    workspace (test_fold_independence_bitwise holds this at cond 1e2; here the direct / deferred
    route choice and the deferred B-half finish act on pivots nine decades apart)."""
    three = sr.graded_inputs(sbce, *shape, 10, sr.SEED, 3)
    idx = np.arange(65) % 3
    inp = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim > 1 else v)
           for k, v in three.items()}

    def solve(nb, **kw):
        th, _, _, st = run(sbce, inp, nb=nb, solve="chol", **kw)
        return bits(th[0]).copy(), int(st[0])

    ref = solve(1)
    assert np.isfinite(ref[0].view(np.float64)).all() and ref[1] == 0
    for what, got in (("batch of 3", solve(3)), ("batch of 65", solve(65)),
                      ("repeat alone", solve(1)), ("repeat, batch of 3", solve(3)),
                      ("ws 0x00", solve(3, ws_fill=0x00)), ("ws 0xFF", solve(3, ws_fill=0xFF)),
                      ("ws 0xFF, batch of 65", solve(65, ws_fill=0xFF))):
        assert np.array_equal(got[0], ref[0]), what
        assert got[1] == ref[1], what
