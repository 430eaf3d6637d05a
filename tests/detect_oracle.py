"""Plain NumPy restatement of the batched detector / soft demapper (include/sbce.h, sbce_detect):
direct distances ||y - H x_j||^2 over all J = M^n_tx hypotheses in itertools.product order and a
max-shifted log-sum-exp per class of hypotheses.  Test infrastructure only: the product has no
CPU path."""
import itertools

import numpy as np


def gray_labeling(M):
    """reflected_2d of "Proposed method/QAM.py":211-217 by its own loop."""
    L = int(round(np.sqrt(M)))
    g = [i ^ (i >> 1) for i in range(L)]
    return np.array([i_I + L * i_Q for i_Q, i_I in itertools.product(g, g)], dtype=np.int32)


def bits_of(labels):
    labels = np.asarray(labels).reshape(-1)
    m = max(int(labels.size - 1).bit_length(), 1)
    return np.array([[(int(l) >> i) & 1 for i in range(m)] for l in labels], dtype=np.int8)


def _lse(z, axis):
    m = np.max(z, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(z - m), axis=axis))


def table_index(cons, x):
    """Index of the table point nearest each entry of x (first minimum)."""
    cons = np.asarray(cons).reshape(-1)
    return np.argmin(np.abs(np.asarray(x)[..., None] - cons) ** 2, axis=-1).astype(np.int32)


def detect_ref(y_d, psi_d, cons, theta, sigma2, n_tx, labels=None, x_d_true=None):
    """y_d (B,T,n_rx), psi_d (B,T,P), cons (M,), theta (B,K), sigma2 scalar or (B,).
    Returns dict(idx (B,T,n_tx) int32, x_hat, post (B,T,n_tx,M), D (B,T) the largest hypothesis
    distance, gap (B,T) relative gap of the two smallest distances [, llr, llr_maxlog
    (B,T,n_tx,log2 M) with labels] [, err (B,2) with x_d_true and labels])."""
    y_d, psi_d, theta = (np.asarray(v, dtype=complex) for v in (y_d, psi_d, theta))
    cons = np.asarray(cons, dtype=complex).reshape(-1)
    B, T, n_rx = y_d.shape
    P, M = psi_d.shape[2], cons.size
    lgM = int(M - 1).bit_length()
    s2 = np.broadcast_to(np.asarray(sigma2, dtype=float).reshape(-1), (B,)) if np.ndim(sigma2) \
        else np.full(B, float(sigma2))
    tab = np.indices((M,) * n_tx).reshape(n_tx, -1).T          # (J, n_tx) table indices
    X = cons[tab]
    out = dict(idx=np.zeros((B, T, n_tx), np.int32), x_hat=np.zeros((B, T, n_tx), complex),
               post=np.zeros((B, T, n_tx, M)), D=np.zeros((B, T)), gap=np.zeros((B, T)))
    bits = None
    if labels is not None:
        bits = bits_of(labels)
        out["llr"] = np.zeros((B, T, n_tx, lgM))
        out["llr_maxlog"] = np.zeros((B, T, n_tx, lgM))
    for b in range(B):
        H = np.einsum("tp,par->tra", psi_d[b], theta[b].reshape(P, n_tx, n_rx))
        d = np.zeros((T, X.shape[0]))
        for t in range(T):
            d[t] = np.sum(np.abs(y_d[b, t][None, :] - X @ H[t].T) ** 2, axis=1)
        j = np.argmin(d, axis=1)
        out["idx"][b] = tab[j]
        out["x_hat"][b] = X[j]
        out["D"][b] = d.max(axis=1)
        if d.shape[1] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            out["gap"][b] = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
        z = -d / s2[b]
        logZ = _lse(z, 1)
        for a in range(n_tx):
            for s in range(M):
                out["post"][b, :, a, s] = np.exp(_lse(z[:, tab[:, a] == s], 1) - logZ)
            if bits is not None:
                for i in range(lgM):
                    one = bits[tab[:, a], i] == 1
                    out["llr"][b, :, a, i] = _lse(z[:, ~one], 1) - _lse(z[:, one], 1)
                    out["llr_maxlog"][b, :, a, i] = (d[:, one].min(axis=1)
                                                     - d[:, ~one].min(axis=1)) / s2[b]
    if x_d_true is not None and labels is not None:
        out["err"] = count_errors(out["idx"], cons, x_d_true, labels)
    return out


def count_errors(idx_hat, cons, x_d_true, labels):
    """(B, 2) int32: symbol entries whose index differs from the true symbol's table index, and
    the differing label bits."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    it = table_index(cons, x_d_true)
    idx_hat = np.asarray(idx_hat)
    B = idx_hat.shape[0]
    x = labels[idx_hat] ^ labels[it]
    nb = np.array([bin(int(v)).count("1") for v in x.reshape(-1)]).reshape(B, -1).sum(axis=1)
    ns = (idx_hat != it).reshape(B, -1).sum(axis=1)
    return np.stack([ns, nb], axis=1).astype(np.int32)


def oracle_detect_batch(y_d, psi_d, cons, theta, varn, n_tx, labels=None, x_d_true=None,
                        noise="em", maxlog=False, want=(), return_device=False):
    """detect_batch's contract computed by the restatement (the sweep only reads 'err')."""
    v = np.asarray(varn, dtype=float)
    r = detect_ref(y_d, psi_d, cons, theta, v * v if noise == "em" else v, n_tx,
                       labels=labels, x_d_true=x_d_true)
    return {"err": r["err"]}
