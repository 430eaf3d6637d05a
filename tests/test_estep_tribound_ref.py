"""The per-group bounds T_3 / T_1 of the V16 sweep as tools/e0_group_bounds.py restates them
(csrc/estep_sweep.hip build_tri: one stream relaxed, tables rounded to float32, the device's margins):
the bound less its margin never exceeds the exact minimum of its tile group, and the sweep with
its running minimum never skips a group that holds a hypothesis inside the final threshold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import e0_group_bounds as gb  # noqa: E402

SNR = 20.0


@pytest.fixture(scope="module")
def cases(sbce):
    """64 symbols (4 trials x 16) of the cfg1 geometry at theta_0 and near the true channel."""
    varn = float(sbce.signal_model.snr_to_varn(SNR))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 64, 16, 16, 16, varn, seed=2)
    out = []
    for name, th in (("theta0", b["theta0"]),
                     ("near", b["h"] + 0.05 * b["theta0"] / np.abs(b["theta0"]).max())):
        H = gb.heff(b, th)
        out += [(name, H[i, t], b["y_d"][i, t], b["cons"], varn, gb.symbol(H[i, t], b["y_d"][i, t], b["cons"], varn))
                for i in range(4) for t in range(16)]
    return out


def test_bound_never_above_its_groups_minimum(cases):
    worst = np.inf
    for name, H, y, cons, varn, r in cases:
        # d[x0, x1, x2, x3] -> the group (blk, kt): x0 in the block, x2 = kt, every x1 and x3
        gmin = r["d"].reshape(4, 4, 16, 16, 16).min(axis=(1, 2, 4))           # [blk, kt]
        for q in (3, 1):
            t = gb.tri_bound(H, y, cons, q)
            assert (t <= gmin).all(), (name, q, float((t - gmin).max()))
            worst = min(worst, float((gmin - t).min() / gmin.max()))
        assert (r["tri"] <= gmin).all(), name
    print(f"smallest (group minimum - bound) / largest group minimum: {worst:.3e}")


def test_bounds_are_not_vacuous(cases):
    """At theta_0 the bounds do remove groups (else the two tests here would show nothing)."""
    n = sum(len(r["skipped"]) for name, *_, r in cases if name == "theta0")
    assert n > 10 * 64, n


@pytest.mark.parametrize("gate", [0, gb.GATE])
def test_no_group_inside_the_final_threshold_is_skipped(cases, gate):
    for name, H, y, cons, varn, r0 in cases:
        r = r0 if gate == 0 else gb.symbol(H, y, cons, varn, gate=gate)
        gmin = r["d"].reshape(4, 4, 16, 16, 16).min(axis=(1, 2, 4))
        thr = gb.THR * varn * varn
        assert r["shift"] <= r["d"].min() + 1e-9 * abs(r["d"].min()) + 1e-300, name   # the minimum was found
        for kt, blk in r["skipped"]:
            assert gmin[blk, kt] > r["d"].min() + thr, (name, kt, blk)
        # the same sweep without the bounds ends at the same running minimum
        assert gb.symbol(H, y, cons, varn, mode="off")["shift"] == r["shift"], name
