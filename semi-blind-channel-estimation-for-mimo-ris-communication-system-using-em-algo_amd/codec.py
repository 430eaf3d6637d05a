"""The binary channel code of the code-aided loop (include/sbce.h sbce_siso_decode): rate-1/n
feed-forward codes, their NumPy encoder and a seeded interleaver.  The decoder is
``em.siso_decode_batch``; this module holds no decoding."""
import numpy as np


class ConvCode:
    """A rate-1/n feed-forward binary code of constraint length K (3..7), n in {2, 3}.

    generators: n K-bit integers (octal literals read naturally: ``ConvCode((0o7, 0o5), 3)``);
    bit K-1 taps the current input, and bit K-1 and bit 0 of every generator must be set.  State
    s = (u_{t-1}, ..., u_{t-K+1}) with u_{t-1} at bit K-2, register word w = (u_t << (K-1)) | s,
    output c_j = parity(w & g_j), next state w >> 1, start state 0.  terminated: K-1 zero tail
    inputs drive the encoder back to state 0 (n_steps = n_info + K - 1); otherwise
    n_steps = n_info."""

    def __init__(self, generators, K, terminated=True):
        self.K = int(K)
        self.generators = tuple(int(g) for g in generators)
        self.terminated = bool(terminated)
        if not 3 <= self.K <= 7:
            raise ValueError("K must lie in 3..7")
        if len(self.generators) not in (2, 3):
            raise ValueError("2 or 3 generators")
        for g in self.generators:
            if g < 0 or g >> self.K or not (g >> (self.K - 1)) & 1 or not g & 1:
                raise ValueError(f"generator {g:o} (octal): bits K-1 and 0 must be set, none above K-1")

    @property
    def n(self):
        return len(self.generators)

    @property
    def n_states(self):
        return 1 << (self.K - 1)

    def n_steps(self, n_info):
        return int(n_info) + (self.K - 1 if self.terminated else 0)

    def n_info_for(self, n_coded):
        """The n_info whose codeword has n_coded bits; ValueError when there is none >= 1."""
        n_coded = int(n_coded)
        steps, rem = divmod(n_coded, self.n)
        n_info = steps - (self.K - 1 if self.terminated else 0)
        if rem or n_info < 1:
            raise ValueError(f"{n_coded} coded bits are no codeword of this code")
        return n_info

    def encode(self, u):
        """(B, n_info) 0/1 -> (B, n_steps * n) int8, coded bit k = t n + j."""
        u = np.asarray(u)
        if u.ndim != 2 or u.shape[1] < 1:
            raise ValueError("u must be (B, n_info) with n_info >= 1")
        if np.any((u != 0) & (u != 1)):
            raise ValueError("u must hold 0/1")
        B, n_info = u.shape
        T = self.n_steps(n_info)
        x = np.zeros((B, T), dtype=np.int64)
        x[:, :n_info] = u
        c = np.zeros((B, T, self.n), dtype=np.int8)
        for j, g in enumerate(self.generators):
            for d in range(self.K):                       # u_{t-d} is tapped by bit K-1-d
                if (g >> (self.K - 1 - d)) & 1:
                    c[:, d:, j] ^= x[:, :T - d].astype(np.int8)
        return c.reshape(B, T * self.n)


def random_interleaver(n, seed):
    """A seeded permutation of 0..n-1 as int32 (``perm`` of em.siso_decode_batch: coded bit k
    travels at position perm[k])."""
    return np.random.default_rng(seed).permutation(int(n)).astype(np.int32)
