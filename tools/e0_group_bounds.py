#!/usr/bin/env python3
"""CPU restatement (numpy arithmetic only; main() takes its batch from the package's numpy
generator signal_model.synthetic_batch, no device and no library) of the V16 E-step sweep's pruning, per symbol of the cfg1 geometry
(n_tx = 4, 16-QAM): which of the 64 tile groups G(kt, tg) -- x_2 = cons[kt], x_0 in
cons[tg .. tg+3], every x_1 and x_3 -- survive the column-tile bound (P-perp of span(h_0, h_1)),
the row-tile bound (P-perp of span(h_1, h_3)) and the per-group bounds T_3 / T_1 (one stream
relaxed) and reach the FP32 screen, and which pass it to the FP64 MFMAs.  The device's best-first
order (visit_order; "natural" is kept for the record), the running minimum starting at the
ridge-rounded candidate, the device's constants (csrc/estep_sweep.hip:
threshold 50 varn^2, ridge 0.1 varn^2, the margins of lb_margin, the screen and build_tri; the
per-group tables rounded to float32 as the device forms them).

Run as a script it rebuilds the tables of profiles/tribound/README.md (natural order) and of
profiles/sweep_order/README.md (both orders):
  python tools/e0_group_bounds.py [snr ...]        (default 20 30 10)
on synthetic_batch(4, 4, 4, 64, 16, 256, 16, varn, seed=2) at theta_0, symbols t = 0, 16, .., 240.
"""
import os
import sys

import numpy as np

THR, RIDGE = 50.0, 0.1          # kSkipThr (csrc/sbce_internal.h), MfmaConst::reg (both times varn^2)
GATE = 4                        # kTriGate


def heff(batch, theta):
    """H_eff (B, T_d, 4, n_rx): row q is stream q's column, sum_p psi_p theta_p."""
    psi = np.asarray(batch["psi_d"])
    B, T, P = psi.shape
    th = np.asarray(theta).reshape(B, P, 4, -1)
    return np.einsum("btp,bpqr->btqr", psi, th)


def _perp(vs, basis):
    """vs minus their components in span(basis) (twice-orthogonalised Gram-Schmidt); None when the
    basis is near-dependent or spans the space."""
    us = []
    for h in basis:
        v = h.copy()
        for _ in range(2):
            for u in us:
                v = v - u * np.vdot(u, v)
        n2, h2 = np.vdot(v, v).real, np.vdot(h, h).real
        if not (h2 > 0.0 and n2 > 1e-6 * h2):
            return None
        us.append(v / np.sqrt(n2))
    out = []
    for v in vs:
        w = v.copy()
        for u in us:
            w = w - u * np.vdot(u, w)
        out.append(w)
    return out


def distances(H, y, cons):
    """d[x0, x1, x2, x3] = ||y - sum_q h_q x_q||^2 in the sweep's own form alpha + gamma - 2 Re p^H q."""
    c = np.asarray(cons)
    pA = y[None, None, :] - c[:, None, None] * H[0] - c[None, :, None] * H[1]      # (16, 16, nr)
    qB = c[:, None, None] * H[2] + c[None, :, None] * H[3]
    al = (np.abs(pA) ** 2).sum(-1)
    ga = (np.abs(qB) ** 2).sum(-1)
    cross = np.einsum("abr,cdr->abcd", pA.conj(), qB).real
    return al[:, :, None, None] + ga[None, None] - 2.0 * cross, al, ga


def tri_bound(H, y, cons, q):
    """The device's bound of stream q in {3, 1} less its margin, as (4, 16) [x_0 block, kt]; zeros
    when the device leaves it at 0.  The tables are rounded to float32 and summed in float32."""
    c = np.asarray(cons)
    o = 4 - q                                            # the other row stream: 1 or 3
    h2 = np.array([np.vdot(h, h).real for h in H])
    cmax2 = (np.abs(c) ** 2).max()
    S = 4.0 * (np.vdot(y, y).real + cmax2 * h2.sum())
    if not (1e-30 < S < 1e30 and h2[q] > 0.0 and h2[q] >= 1e-20 * h2.max()):
        return np.zeros((4, 16))
    proj = lambda v: v - H[q] * (np.vdot(H[q], v) / h2[q])
    py, p0, po, p2 = proj(y), proj(H[0]), proj(H[o]), proj(H[2])
    ri = lambda z: np.stack([z.real, z.imag], -1).reshape(z.shape[0], -1)      # (16, 2 nr)
    U = -2.0 * ri(py[None, :] - c[:, None] * p0[None, :])
    V = 2.0 * ri(c[:, None] * po[None, :])
    Q = ri(c[:, None] * p2[None, :])
    uu, vv, qq = (U * U).sum(1), (V * V).sum(1), (Q * Q).sum(1)
    U32, V32, Q32 = U.astype(np.float32), V.astype(np.float32), Q.astype(np.float32)
    al32 = (0.5 * (U32 @ V32.T).astype(np.float64) + 0.25 * (uu[:, None] + vv[None, :])).astype(np.float32)
    A32 = U32[:, None, :] + V32[None, :, :]                                      # (x0, xo, 2 nr)
    T32 = al32[:, :, None] + np.einsum("abk,ck->abc", A32, Q32).astype(np.float32)
    tmin = T32.min(axis=1).astype(np.float64)                                    # (x0, kt)
    margin = 2.0 ** -16 * (2.0 * 0.5 * (uu.max() + vv.max()) + qq) + 1e-9 * S
    return tmin.reshape(4, 4, 16).min(axis=1) + qq[None, :] - margin[None, :]


def visit_order(lb, rb, order="device", margin=0.0):
    """The soft sweep's visiting order: the column tiles, and per column tile its four row blocks.
    'device': column tiles by ascending column-tile bound lb[kt], the row blocks of tile kt by
    ascending block minimum of the row-tile bound rb[s0, kt], ties to the smaller index (stable),
    a bound below `margin` (the device's lb_margin) counting as 0;
    'natural': 0, 1, 2, ... (the order before best-first, and the hard decision's)."""
    if order == "natural":
        return list(range(16)), [list(range(4))] * 16
    if order != "device":
        raise ValueError(order)
    key = lambda v: np.where(v < margin, 0.0, v)         # a bound below its rounding margin ties at 0
    kts = [int(k) for k in np.argsort(key(lb), kind="stable")]
    blks = [[int(b) for b in np.argsort(key(rb[:, kt].reshape(4, 4).min(axis=1)), kind="stable")]
            for kt in range(16)]
    return kts, blks


def symbol(H, y, cons, varn, mode="both", gate=0, thr_scale=1.0, order="device"):
    """One symbol's soft sweep.  mode: 'off' (column- and row-tile bounds only), 't3' (third-stream
    bound only) or 'both'; gate: groups at the screen before the tables exist (0: from the start);
    order: visit_order's.  As on the device the column-tile bound is tested when a tile is reached
    (in the device's order the first tile above the limit ends the symbol), the row-tile test is
    made once on entering a column tile, and the per-group bound and the screen are tested as each
    block is reached.  Returns a dict: screen / fp64 group counts, within (hypotheses inside the
    final threshold), skipped (set of (kt, blk) the per-group bounds removed), swept (set of
    (kt, blk) that ran in FP64), shift (the final running minimum), d."""
    c = np.asarray(cons)
    nr = len(y)
    d, al, ga = distances(H, y, c)
    thr = THR * varn * varn * thr_scale
    # the ridge-rounded candidate
    Hm = H.T                                             # (nr, 4)
    z = np.linalg.solve(Hm.conj().T @ Hm + RIDGE * varn * varn * np.eye(4), Hm.conj().T @ y)
    xc = [int(np.argmin(np.abs(zq - c) ** 2)) for zq in z]
    cscale = np.vdot(y, y).real + 4.0 * sum((np.abs(H[q] * c[xc[q]]) ** 2).sum() for q in range(4))
    shift = d[tuple(xc)] + 1e-10 * cscale
    # column-tile bounds and their margin
    cmax2 = (np.abs(c) ** 2).max()
    lbm = 1e-9 * (np.vdot(y, y).real + 2.0 * cmax2 * ((np.abs(H[2]) ** 2).sum() + (np.abs(H[3]) ** 2).sum()))
    lb = np.zeros(16)
    pp = _perp([y, H[2], H[3]], [H[0], H[1]]) if nr > 2 else None
    if pp is not None:
        res = pp[0][None, None, :] - c[:, None, None] * pp[1] - c[None, :, None] * pp[2]
        lb = (np.abs(res) ** 2).sum(-1).min(axis=1)
    # row-tile bounds: ||P y - x_s0 P h_0 - x_kt P h_2||^2, P-perp of span(h_1, h_3)
    rb = np.zeros((16, 16))                              # [s0, kt]
    pr = _perp([y, H[0], H[2]], [H[1], H[3]]) if nr > 2 else None
    if pr is not None:
        res = pr[0][None, None, :] - c[:, None, None] * pr[1] - c[None, :, None] * pr[2]
        rb = (np.abs(res) ** 2).sum(-1)
    tri = np.zeros((4, 16))
    if mode != "off":
        tri = np.maximum(tri, tri_bound(H, y, c, 3))
        if mode == "both":
            tri = np.maximum(tri, tri_bound(H, y, c, 1))
    amax = al.max()
    gmin = d.reshape(4, 4, 16, 16, 16).min(axis=(1, 2))  # [blk, kt, x3]: group minima per column
    screen = fp64 = scr_n = scr_pass = 0
    scr_on, have = True, False
    skipped, swept = set(), set()
    kts, blks = visit_order(lb, rb, order, lbm)
    for kt in kts:
        if lb[kt] > shift + thr + lbm:
            if order == "device":
                break                # the bounds ascend, the limit only falls
            continue
        if mode != "off" and not have and screen >= gate:
            have = True
        rows = rb[:, kt] <= shift + thr + lbm
        # blocks the row bound admits and the per-group bound rejects on entering the tile: they
        # count as rejections in the screen's pass rate (so do the ones rejected when reached)
        dead = [blk for blk in range(4) if have and rows[4 * blk:4 * blk + 4].any() and tri[blk, kt] > shift + thr]
        skipped.update((kt, blk) for blk in dead)
        if scr_on:
            scr_n += len(dead)
        for blk in blks[kt]:
            if not rows[4 * blk:4 * blk + 4].any() or blk in dead:
                continue
            if have and tri[blk, kt] > shift + thr:
                skipped.add((kt, blk))
                scr_n += scr_on
                continue
            screen += 1
            gm = gmin[blk, kt]
            if scr_on:
                scr_n += 1
                ok = (gm <= shift + thr + 2.0 ** -17 * (2.0 * amax + ga[kt])).any()
                scr_pass += ok
                if scr_n >= 16 and 2 * scr_pass > scr_n:
                    scr_on = False
                if not ok:
                    continue
            fp64 += 1
            swept.add((kt, blk))
            if gm.min() <= shift + thr:
                shift = min(shift, gm.min())
    return dict(screen=screen, fp64=fp64, within=int((d <= d.min() + thr).sum()), skipped=skipped,
                swept=swept, shift=shift, d=d, tri=tri, lb=lb, rb=rb)


def count_groups(batch, theta, varn, tri=True, gate=0, symbols=None, order="device"):
    """Totals over the batch's symbols (or the (b, t) pairs given) of the groups that reach the
    screen and of the FP64 groups, as the device's counters count them (order: visit_order's)."""
    H = heff(batch, theta)
    y = np.asarray(batch["y_d"])
    if symbols is None:
        symbols = [(b, t) for b in range(H.shape[0]) for t in range(H.shape[1])]
    tot = dict(screen=0, fp64=0, within=0, symbols=len(symbols))
    for b, t in symbols:
        r = symbol(H[b, t], y[b, t], batch["cons"], varn, "both" if tri is True else (tri or "off"), gate,
                   order=order)
        for k in ("screen", "fp64", "within"):
            tot[k] += r[k]
    return tot


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    sm = ge.package().signal_model
    snrs = [float(s) for s in sys.argv[1:]] or [20.0, 30.0, 10.0]
    print("per listed symbol (4 trials x 16 symbols, theta_0)")
    print(f"{'SNR dB':>7} {'within thr':>11} {'to screen':>10} {'FP64':>6} {'T3+T1':>7} {'T3 only':>8} {'gated':>7}")
    for snr in snrs:
        varn = float(sm.snr_to_varn(snr))
        b = sm.synthetic_batch(4, 4, 4, 64, 16, 256, 16, varn, seed=2)
        sy = [(i, t) for i in range(4) for t in range(0, 256, 16)]
        n = len(sy)
        for order in ("natural", "device"):
            off = count_groups(b, b["theta0"], varn, tri=False, symbols=sy, order=order)
            both = count_groups(b, b["theta0"], varn, tri=True, symbols=sy, order=order)
            t3 = count_groups(b, b["theta0"], varn, tri="t3", symbols=sy, order=order)
            gated = count_groups(b, b["theta0"], varn, tri=True, gate=GATE, symbols=sy, order=order)
            print(f"{snr:7.0f} {off['within'] / n:11.1f} {off['screen'] / n:10.1f} {off['fp64'] / n:6.1f} "
                  f"{both['screen'] / n:7.1f} {t3['screen'] / n:8.1f} {gated['screen'] / n:7.1f}"
                  f"   {order} order: FP64 groups {both['fp64'] / n:.2f} (T3+T1), {gated['fp64'] / n:.2f} (gated)")


if __name__ == "__main__":
    main()
