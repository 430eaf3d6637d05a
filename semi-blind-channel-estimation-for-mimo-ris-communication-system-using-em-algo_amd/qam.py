"""QAM constellation tables in the order of the reference's vendored ``komm``
QAModulation ("Proposed method/QAM.py":306-322): square M = L^2, base amplitude 1,
in-phase index fastest:  s -> (2*(s % L) - L + 1) + 1j*(2*(s // L) - L + 1).

This order fixes the hypothesis enumeration (``itertools.product`` over this
table, "Proposed method/Proposed_method_NMSEvsTp.py":32-38) and the symbol draws
(``qamCons[np.random.choice(range(M), n_tx, 'True')]``, :31).
"""
import numpy as np


def qam_constellation(M):
    L = int(round(np.sqrt(M)))
    if L * L != M or L & (L - 1):
        raise ValueError("M must be a square power of two (4, 16, 64, 256)")
    ci = np.arange(-L + 1, L, 2, dtype=np.int64).astype(float)
    cq = np.arange(-L + 1, L, 2, dtype=np.int64).astype(float)
    return (ci + 1j * cq[:, None]).reshape(-1)


def energy_per_symbol(M):
    """E_s = mean |s|^2 ("Proposed method/QAM.py":81): 2, 10, 42 for 4/16/64-QAM."""
    c = qam_constellation(M)
    return float(np.mean(c.real ** 2 + c.imag ** 2))


def gray_labeling(M):
    """The reference modem's default binary labelling of the square table above: 'reflected_2d'
    ("Proposed method/QAM.py":211-217), label = gray(i_I) + L * gray(i_Q) for the point with
    in-phase index i_I and quadrature index i_Q (table index s = i_I + L * i_Q)."""
    L = int(round(np.sqrt(M)))
    if L * L != M or L & (L - 1):
        raise ValueError("M must be a square power of two (4, 16, 64, 256)")
    g = np.arange(L, dtype=np.int64)
    g ^= g >> 1
    return (g[None, :] + L * g[:, None]).reshape(-1).astype(np.int32)


def bits_of(labels):
    """(M, log2 M) array of the labels' bits, LSB first (QAM.py:8-11, :31)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    m = max(int(labels.size - 1).bit_length(), 1)
    return ((labels[:, None] >> np.arange(m)[None, :]) & 1).astype(np.int8)


def map_bits(bits, cons, labels):
    """Bits to table points: bits (..., log2 M) of 0/1, LSB first under ``labels`` -> (...) complex,
    the point s with bits_of(labels)[s] == bits; the inverse of ``bits_of(labels)[idx]``."""
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    bits = np.asarray(bits)
    m = max(int(cons.size - 1).bit_length(), 1)
    if labels.size != cons.size or bits.shape[-1] != m:
        raise ValueError(f"bits must end in log2 M = {m} and labels have M = {cons.size} entries")
    if np.any((bits != 0) & (bits != 1)) or not np.array_equal(np.sort(labels), np.arange(cons.size)):
        raise ValueError("bits must be 0/1 and labels a permutation of 0..M-1")
    index_of = np.empty(cons.size, dtype=np.int64)
    index_of[labels] = np.arange(cons.size)
    word = (bits.astype(np.int64) << np.arange(m)).sum(axis=-1)
    return cons[index_of[word]]


def prior_llr_known(x, cons, labels):
    """A-priori bit L-values log(P(bit = 0) / P(bit = 1)) that mark the symbols ``x`` (any shape,
    each the table point nearest to it) as known: +inf where the symbol's bit is 0, -inf where it
    is 1; shape x.shape + (log2 M,).  The library clamps them to +-64 (include/sbce.h)."""
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    x = np.asarray(x, dtype=complex)
    idx = np.argmin(np.abs(x[..., None] - cons), axis=-1)
    return np.where(bits_of(labels)[idx] == 0, np.inf, -np.inf)


_J_H1, _J_H2, _J_H3 = 0.3073, 0.8935, 1.1064


def _j_inverse(i_a):
    """sigma with J(sigma) = i_a for J(sigma) ~ (1 - 2^(-H1 sigma^(2 H2)))^H3, the usual closed
    form of the consistent-Gaussian L-value's mutual information (2 H2 = 1.787)."""
    return (-np.log2(1.0 - i_a ** (1.0 / _J_H3)) / _J_H1) ** (1.0 / (2.0 * _J_H2))


def prior_llr_gaussian(bits, i_a, rng):
    """The consistent-Gaussian a-priori model of EXIT analysis: La = (1 - 2 b) sigma^2 / 2 +
    sigma n with n ~ N(0, 1) from ``rng`` (a numpy Generator or RandomState) and sigma =
    J^-1(i_a), for the 0/1 array ``bits``.  i_a = 0 gives all zeros, i_a = 1 gives +-inf."""
    bits = np.asarray(bits)
    i_a = float(i_a)
    if not 0.0 <= i_a <= 1.0:
        raise ValueError("i_a must lie in [0, 1]")
    sign = 1.0 - 2.0 * bits
    if i_a == 0.0:
        return np.zeros(bits.shape)
    if i_a == 1.0:
        return np.where(bits == 0, np.inf, -np.inf)
    sigma = _j_inverse(i_a)
    return sign * (sigma * sigma / 2.0) + sigma * rng.standard_normal(bits.shape)


def bit_mutual_information(llr, bits):
    """1 - mean log2(1 + e^{-(1 - 2 b) L}): the mutual information between the bits and their
    L-values log(P(bit = 0) / P(bit = 1)), by the time average."""
    z = -(1.0 - 2.0 * np.asarray(bits)) * np.asarray(llr, dtype=float)
    return float(1.0 - np.mean(np.logaddexp(0.0, z)) / np.log(2.0))


def all_possible_symbols(cons, n_tx):
    """J = M^n_tx hypotheses in itertools.product order (first stream slowest)."""
    cons = np.asarray(cons)
    M = cons.size
    idx = np.indices((M,) * n_tx).reshape(n_tx, -1).T
    return cons[idx]
