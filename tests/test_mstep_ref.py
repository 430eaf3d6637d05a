"""CPU tier: the extended-precision M-step restatement (tests/mstep_ref.py) against the float64
oracle under the bound the device is held to, the properties its generator promises, and the
restated staging-segment rule of rbuild_herm_kernel against a brute-force index count."""
import numpy as np
import pytest

import mstep_ref as mr
from conftest import rel
from oracle.em_reduced import mstep_build, mstep_build_gemm


@pytest.mark.parametrize("shape", [
    # (n_tx, n_rx, P, T_p, T_d)
    (4, 2, 22, 3, 19), (8, 3, 11, 3, 19), (3, 6, 22, 1, 1), (5, 4, 13, 3, 30), (7, 2, 10, 1, 17),
    (1, 8, 300, 3, 19), (2, 2, 125, 3, 33), (6, 5, 30, 6, 60),
])
def test_restatement_matches_oracle_under_the_bound(shape):
    n_tx, n_rx, P, T_p, T_d = shape
    b = mr.general_batch(2, n_tx, n_rx, P, T_p, T_d, seed=17)
    for i, (R, rhs, R_abs, rhs_abs) in enumerate(mr.batch_ref(b)):
        args = (b["u_p"][i], b["y_p"][i], b["psi_d"][i].T, b["y_d"][i], b["m"][i], b["S"][i])
        for build in (mstep_build, mstep_build_gemm):
            R0, rhs0 = build(*args)
            rr, rb = mr.ratio(R0, R, T_p, T_d, R_abs), mr.ratio(rhs0, rhs, T_p, T_d, rhs_abs)
            print(f"{shape} {build.__name__}: err / bound R {rr:.3f} rhs {rb:.3f}")
            assert rr <= 1.0 and rb <= 1.0
            assert rel(R0, R.astype(complex)) < 1e-13 and rel(rhs0, rhs.astype(complex)) < 1e-13
        assert R.dtype == mr.CLD and rhs.dtype == mr.CLD
        assert R_abs.dtype == np.float64 and rhs_abs.dtype == np.float64
        # the triangle inequality, entry by entry: the bound's scale is never below the entry
        assert (np.abs(R).astype(float) <= R_abs * (1 + 1e-12)).all()
        assert (np.abs(rhs).astype(float) <= rhs_abs * (1 + 1e-12)).all()


def test_bound_is_the_stated_one():
    a = np.array([[2.0, 0.5]])
    assert np.array_equal(mr.bound(3, 19, a), 30 * 2.0 ** -53 * a)
    ref = np.array([1.0 + 0j], dtype=mr.CLD)
    dev = np.array([1.0 + 30 * 2.0 ** -53 + 0j])
    assert mr.ratio(dev, ref, 3, 19, np.array([1.0])) == pytest.approx(1.0, rel=1e-12)


@pytest.mark.parametrize("shape", [(4, 2, 9, 3, 19), (7, 3, 5, 2, 11), (1, 1, 30, 1, 4)])
def test_reference_is_hermitian(shape):
    n_tx, n_rx, P, T_p, T_d = shape
    b = mr.general_batch(2, n_tx, n_rx, P, T_p, T_d, seed=3, break_trial=1)
    for R, _, R_abs, _ in mr.batch_ref(b):
        # symmetric to the restatement's own rounding: the bound of the module docstring with the
        # extended format's unit roundoff 2^-64, once for each of the two entries
        assert (np.abs(R - np.conj(R.T)).astype(float)
                <= 2 * (T_p + T_d + 8) * 2.0 ** -64 * R_abs).all()
        assert np.allclose(R_abs, R_abs.T, rtol=1e-14, atol=0)     # float64 sums, any order
        assert (R.diagonal().real > 0).all()


@pytest.mark.parametrize("n_tx", [1, 2, 3, 4, 5, 6, 7, 8])
def test_generator_moments_are_general(n_tx):
    b = mr.general_batch(3, n_tx, 2, 6, 3, 12, seed=n_tx, break_trial=2)
    S, psi = b["S"], b["psi_d"]
    assert np.array_equal(S, np.conj(np.swapaxes(S, -1, -2)))              # exactly Hermitian
    assert (np.linalg.eigvalsh(S) >= 0.1 * (1 - 1e-9)).all()               # A A^H + 0.1 I
    d = np.real(np.einsum("btaa->bta", S))
    assert np.array_equal(np.imag(np.einsum("btaa->bta", S)), np.zeros_like(d))
    for row in d.reshape(-1, n_tx):
        assert len(set(row.tolist())) == n_tx                              # distinct diagonals
    if n_tx > 1:
        off = S[..., 0, 1]
        assert (np.abs(off.real) > 0).all() and (np.abs(off.imag) > 0).all()
    assert np.allclose(np.abs(psi), 1.0, rtol=0, atol=1e-15) and (psi[..., 0] == 1).all()
    assert (b["psi_p"][..., 0] == 1).all()
    kron = np.einsum("btp,bta->btpa", b["psi_p"], b["x_p"]).reshape(b["u_p"].shape)
    assert np.array_equal(b["u_p"][:2], kron[:2])
    assert np.abs(b["u_p"][2] - kron[2]).max() > 1e-2                      # the broken trial


HERM_TABLE = {
    # (P, pairs per block): (layouts, largest staged count, blocks)
    (1, 256): ({"row"}, 1, 1),
    (22, 256): ({"prefix"}, 22, 1),
    (23, 256): ({"prefix", "row"}, 23, 2),
    (65, 256): ({"prefix"}, 65, 9),
    (68, 256): ({"prefix", "row"}, 68, 10),
    (258, 256): ({"prefix", "row", "two_rows"}, 257, 131),
    (300, 256): ({"prefix", "row", "row+p", "two_rows"}, 257, 177),
    (11, 64): ({"prefix", "row"}, 11, 2),
    (64, 64): ({"prefix", "row"}, 64, 33),
    (65, 64): ({"prefix", "row"}, 65, 34),
    (66, 64): ({"prefix", "row", "two_rows"}, 65, 35),
    (81, 64): ({"prefix", "row", "row+p", "two_rows"}, 65, 52),
}


@pytest.mark.parametrize("key", sorted(HERM_TABLE))
def test_herm_segments_table_and_coverage(key):
    """The table, and for every block by brute force: the two segments are ordered and disjoint,
    hold every p and q of the block's pairs, and count at most min(P, pairs per block + 1)."""
    P, ppb = key
    s = mr.herm_segments(P, ppb)
    assert (s["layouts"], s["count"], len(s["blocks"])) == HERM_TABLE[key]
    assert s["layouts"] <= set(mr.LAYOUTS)
    assert s["count"] <= min(P, ppb + 1)
    for name, lo1, hi1, lo2, hi2, pi0, pi1 in s["blocks"]:
        assert 0 <= lo1 <= hi1 < lo2 <= hi2 + 1 <= P
        staged = set(range(lo1, hi1 + 1)) | set(range(lo2, hi2 + 1))
        need = {x for pi in range(pi0, pi1 + 1) for x in mr.pair_of(pi)}
        assert need <= staged, name
        assert (name in ("row", "prefix")) == (lo2 > hi2)
    pairs = [mr.pair_of(pi) for pi in range(P * (P + 1) // 2)]
    assert pairs == [(p, q) for p in range(P) for q in range(p + 1)]
