"""CPU tier: the helper tests/solve_ref.py itself.

  * chol_solve_ld against a 40-digit mpmath Cholesky: its extra digits are real;
  * the float64 restatement of the device's solve (oracle.em_reduced.mstep_chol_policy) on
    every (shape, decades) tests/test_gpu_chol_cond.py runs meets the bars that file holds the
    device to, drops no pivot and keeps its smallest pivot >= 1e3 tol: the inputs make the bars
    attainable (a seed that violates a condition is changed, never the bar);
  * planted_inputs: the restatement drops exactly the planted block.

Every case prints its margins; run with -s to read them.
"""
import functools

import numpy as np
import pytest

import solve_ref as sr
from conftest import rel


# ------------------------------------------------------------------ 40 digits
def _mp_solve(R, rhs):
    """R X = rhs by an unblocked Cholesky in 40-digit mpmath arithmetic: X as clongdouble."""
    import mpmath as mp
    with mp.workdps(40):
        L, nr = rhs.shape
        A = [[mp.mpc(R[i, j].real, R[i, j].imag) if i != j else mp.mpc(R[i, i].real, 0)
              for j in range(L)] for i in range(L)]
        G = [[mp.mpc(0)] * L for _ in range(L)]
        for c in range(L):
            d = A[c][c].real - sum((abs(G[c][k]) ** 2 for k in range(c)), mp.mpf(0))
            G[c][c] = mp.mpc(mp.sqrt(d), 0)
            for i in range(c + 1, L):
                acc = A[i][c] - sum((G[i][k] * mp.conj(G[c][k]) for k in range(c)), mp.mpc(0))
                G[i][c] = acc / G[c][c]
        X = np.zeros((L, nr), dtype=sr.CLD)
        for r in range(nr):
            y = [mp.mpc(0)] * L
            for c in range(L):
                acc = mp.mpc(rhs[c, r].real, rhs[c, r].imag)
                y[c] = (acc - sum((G[c][k] * y[k] for k in range(c)), mp.mpc(0))) / G[c][c]
            x = [mp.mpc(0)] * L
            for c in range(L - 1, -1, -1):
                acc = y[c] - sum((mp.conj(G[k][c]) * x[k] for k in range(c + 1, L)), mp.mpc(0))
                x[c] = acc / G[c][c]
            for c in range(L):
                # two long doubles per part: the float64 head and the remainder
                re, im = x[c].real, x[c].imag
                X[c, r] = (sr.LD(float(re)) + sr.LD(float(re - mp.mpf(float(re))))) + \
                    1j * (sr.LD(float(im)) + sr.LD(float(im - mp.mpf(float(im)))))
        return X


@pytest.mark.parametrize("shape", [(2, 2, 7), (4, 3, 3), (3, 2, 4), (1, 4, 12)])
@pytest.mark.parametrize("decades", [4, 10])
def test_chol_solve_ld_against_mpmath(sbce, shape, decades):
    """L <= 16: the long-double solve is within 1e-15 cond 1e-3 of the 40-digit one, a thousand
    times below the smallest forward bar it serves as the reference for."""
    n_tx, n_rx, N = shape
    inp = sr.graded_inputs(sbce, n_tx, n_rx, N, decades, sr.SEED, 1)
    R, rhs = sr.host_system(inp, 0)
    assert R.shape[0] <= 16
    theta, dropped, piv = sr.chol_solve_ld(R, rhs)
    assert not dropped.any()
    want = np.conj(_mp_solve(sr.herm_lower(R, np.complex128), rhs)).reshape(-1)
    cond = np.linalg.cond(R)
    err = sr.rel_ld(theta, want)
    print(f"[solve-ref] mpmath {shape} decades {decades}: cond {cond:.2e} "
          f"err {err:.2e} = {err / (float(np.finfo(sr.LD).eps) * cond):.3f} eps_ld cond")
    assert 10.0 ** (decades - 1) < cond < 10.0 ** (decades + 1.5)
    assert err < 1e-15 * cond * 1e-3


def test_chol_solve_ld_policy_and_completion():
    """The pivot rule (a zero Schur complement is dropped, its unknowns 0, the rest solved) and
    the Hermitian completion: the strict upper triangle and the diagonal's imaginary part of the
    R it is given are not read."""
    g = np.random.default_rng(5)
    A = sr._cn(g, (6, 4))
    R = A @ A.conj().T                        # rank 4: the last two pivots are rounding noise
    rhs = R @ sr._cn(g, (6, 2))
    theta, dropped, piv = sr.chol_solve_ld(R, rhs)
    assert dropped.tolist() == [False] * 4 + [True] * 2
    assert np.all(theta.reshape(6, 2)[4:] == 0)
    assert sr.backward_error(R, theta, rhs, 2) < 1e-15
    junk = np.tril(R) + np.triu(sr._cn(g, (6, 6)), 1) + 1j * np.diag(g.standard_normal(6))
    theta2, dropped2, piv2 = sr.chol_solve_ld(junk, rhs)
    assert np.array_equal(theta, theta2) and np.array_equal(piv, piv2)
    from oracle.em_reduced import mstep_chol_policy
    th64, bad = mstep_chol_policy(R, rhs)
    assert np.array_equal(bad, dropped)
    assert sr.rel_ld(th64, theta) < 1e-10


# ------------------------------------------------------------------ the GPU tier's inputs
@functools.lru_cache(maxsize=None)
def _graded(sbce, shape, decades):
    return sr.graded_inputs(sbce, *shape, decades, sr.SEED, sr.trials_of(shape))


@pytest.mark.parametrize("shape", sr.SHAPES)
def test_restatement_meets_the_gpu_bars(sbce, shape):
    """Every (shape, decades) of the GPU tier, on the oracle's R and B^H: the float64
    restatement against chol_solve_ld meets the forward bar max(1e-12, 1e-15 cond) and the
    backward bar 8 eps, flags nothing, and its smallest pivot is >= 1e3 tol; cond_2(R) is
    10^decades times a small factor; SBCE_STATUS_PILOT's premise (Kronecker pilots) holds."""
    n_tx, n_rx, N = shape
    for decades in sr.decades_of(shape):
        inp = _graded(sbce, shape, decades)
        assert inp["T_d"] == inp["P"] == N + 1 and inp["T_p"] == sr.T_P
        for i in range(sr.trials_of(shape)):
            R, rhs = sr.host_system(inp, i)
            ref = sr.reference(R, rhs, n_rx)
            err = sr.rel_ld(ref["th_cpu"], ref["theta"])
            pmin = float(ref["piv"].min())
            print(f"[solve-ref] {shape} L={inp['L']} decades {decades} trial {i}: "
                  f"cond {ref['cond']:.2e} err/(eps cond) {err / (sr.EPS * ref['cond']):.4f} "
                  f"eta/eps {ref['eta_cpu'] / sr.EPS:.3f} min pivot/tol {pmin / ref['tol']:.2e} "
                  f"min pivot/max diag {pmin * sr.REL_TOL / ref['tol']:.2e}")
            assert 10.0 ** (decades - 1) < ref["cond"] < 10.0 ** (decades + 1.5)
            assert not ref["dropped"].any() and not ref["bad_cpu"].any()
            assert pmin >= 1e3 * ref["tol"]
            assert np.isfinite(ref["th_cpu"]).all()
            assert err <= sr.forward_bar(ref["cond"])
            assert ref["eta_cpu"] <= 8 * sr.EPS
            # the pilot term is rounding-level against R's smallest eigenvalue, yet not zero
            up = inp["u_p"][i]
            assert 0 < np.abs(up).max() ** 2 * sr.T_P < 1e-4 * inp["s"].min()


def test_graded_inputs_are_what_they_say(sbce):
    """psi_d[b] is Q^T with Q unitary and different per trial, S_t is exactly Hermitian with the
    eigenvalues s_t and s_t (1 + |v_t|^2 / 2), and R has the eigenvalues of the S_t."""
    inp = sr.graded_inputs(sbce, 3, 2, 9, 7, sr.SEED, 2)
    P = 10
    for i in range(2):
        Q = inp["psi_d"][i].T
        assert rel(Q.conj().T @ Q, np.eye(P)) < 1e-14
    assert rel(inp["psi_d"][0], inp["psi_d"][1]) > 0.1
    S = inp["S"]
    assert np.array_equal(S, np.conj(np.swapaxes(S, -1, -2)))
    assert np.array_equal(inp["s"][0], np.logspace(0, -7, P))
    ev = np.sort(np.concatenate([np.linalg.eigvalsh(S[0, t]) for t in range(P)]))
    assert np.all(ev > 0)
    up0 = inp["u_p"][0]
    inp["u_p"][0] = 0
    R, _ = sr.host_system(inp, 0)
    inp["u_p"][0] = up0
    assert np.allclose(np.linalg.eigvalsh(R), ev, rtol=1e-6, atol=0)


# ------------------------------------------------------------------ planted pivots
def test_tiny_positions_reach_the_boundaries():
    """The positions are distinct blocks inside the system, a block straddles column 16 and
    column 32 where n_tx = 3, and the remainder position lies in the last panel."""
    for shape in sr.SHAPES:
        n_tx, n_rx, N = shape
        pos = sr.tiny_positions(shape)
        assert len(set(pos.values())) == len(pos) and all(0 <= b <= N for b in pos.values())
        assert "col0" in pos and pos[max(pos, key=pos.get)] == N
    pos = sr.tiny_positions((3, 4, 22))
    assert (pos["edge16"], pos["edge32"]) == (5, 10)        # columns 15..17 and 30..32
    assert sr.tiny_positions((3, 2, 200))["edge64"] == 21   # columns 63..65
    assert sr.tiny_positions((4, 2, 64))["remainder"] == 64 # columns 256..259, the folded panel
    assert sr.tiny_positions((4, 2, 74))["remainder"] == 72 # columns 288..291 of 288..299


@pytest.mark.parametrize("shape", sr.SHAPES)
def test_planted_mask_is_what_the_restatement_drops(sbce, shape):
    """Every planted case of the GPU tier: R is block diagonal to 1e-40 of its smallest block,
    the big block holds the largest diagonal entry, every diagonal entry of the tiny block is
    >= 100 times below tol and every Cholesky pivot of the other blocks >= 100 times above, and
    the float64 restatement and chol_solve_ld, run on the whole R, drop exactly the planted
    block, in trial 0 only.  (Above L = 512 a whole-R run costs seconds: there two of the
    positions get it and every position the per-block pivots, which for a block-diagonal R are
    the whole-R pivots.)"""
    from oracle.em_reduced import mstep_chol_policy
    n_tx, n_rx, N = shape
    P = N + 1
    blocks = np.kron(np.eye(P), np.ones((n_tx, n_tx))) > 0
    whole = 0
    for big in ("first", "last"):
        for name, blk in sr.tiny_positions(shape).items():
            s, big_block = sr.planted_scales(shape, big, blk)
            inp = sr.planted_inputs(sbce, n_tx, n_rx, N, s, sr.SEED)
            mask = sr.planted_mask(shape, blk)
            run_whole = sr.family(shape) != "large" or (big, name) in (("first", "edge64"),
                                                                       ("last", "remainder"))
            for i in range(2):
                R, rhs = sr.host_system(inp, i)
                assert np.abs(R[~blocks]).max(initial=0.0) <= 1e-40 * sr.S_TINY
                d = R.diagonal().real
                tol = sr.REL_TOL * d.max()
                assert d.argmax() // n_tx == big_block
                want = mask if i == 0 else np.zeros_like(mask)
                keep = [t for t in range(P) if not (i == 0 and t == blk)]
                Rb = R.reshape(P, n_tx, P, n_tx)
                G = np.linalg.cholesky(np.stack([Rb[t, :, t, :] for t in keep]))
                piv = np.real(np.einsum("tii->ti", G)) ** 2
                assert piv.min() >= 100 * tol, (big, name, i)
                if i == 0:
                    assert d[mask].max() <= tol / 100
                if run_whole:
                    whole += 1
                    _, bad = mstep_chol_policy(R, rhs)
                    _, dropped, piv_ld = sr.chol_solve_ld(R, rhs)
                    assert np.array_equal(bad, want), (big, name, i)
                    assert np.array_equal(dropped, want), (big, name, i)
                    assert float(piv_ld[~want].min()) >= 100 * tol
            print(f"[solve-ref] planted {shape} big {big} ({big_block}) tiny {name} ({blk}): ok")
    assert whole >= 4
