"""The V16 soft sweep's best-first order as tools/e0_group_bounds.py restates it (visit_order:
column tiles by ascending column-tile bound, the first one above the limit ending the symbol; the
row blocks of a tile by ascending block minimum of the row-tile bound): the sweep still ends at the
true minimum, skips no group that holds a hypothesis inside the final threshold, and runs fewer
FP64 groups at theta_0 than the natural order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import e0_group_bounds as gb  # noqa: E402

SNR = 20.0


@pytest.fixture(scope="module")
def cases(sbce):
    """64 symbols (4 trials x 16) of the cfg1 geometry at theta_0 and near the true channel, swept
    in the device's order and in the natural one."""
    varn = float(sbce.signal_model.snr_to_varn(SNR))
    b = sbce.signal_model.synthetic_batch(4, 4, 4, 64, 16, 16, 16, varn, seed=2)
    out = []
    for name, th in (("theta0", b["theta0"]),
                     ("near", b["h"] + 0.05 * b["theta0"] / np.abs(b["theta0"]).max())):
        H = gb.heff(b, th)
        for i in range(4):
            for t in range(16):
                a = (H[i, t], b["y_d"][i, t], b["cons"], varn)
                out.append((name, a, gb.symbol(*a), gb.symbol(*a, order="natural")))
    return out


def test_default_order_is_the_devices(cases):
    name, a, r, nat = cases[0]
    assert gb.symbol(*a, order="device")["swept"] == r["swept"]
    kts, blks = gb.visit_order(r["lb"], r["rb"])
    assert sorted(kts) == list(range(16)) and all(sorted(x) == [0, 1, 2, 3] for x in blks)
    assert all(r["lb"][kts[n]] <= r["lb"][kts[n + 1]] for n in range(15))
    # equal bounds: the natural order
    assert gb.visit_order(np.zeros(16), np.zeros((16, 16))) == gb.visit_order(None, None, "natural")


@pytest.mark.parametrize("gate", [0, gb.GATE])
@pytest.mark.parametrize("mode", ["both", "off"])
def test_ends_at_the_true_minimum_and_skips_nothing_inside_the_threshold(cases, gate, mode):
    for name, a, r0, nat in cases:
        r = r0 if (gate == 0 and mode == "both") else gb.symbol(*a, mode=mode, gate=gate)
        dmin = r["d"].min()
        thr = gb.THR * a[3] * a[3]
        assert r["shift"] <= dmin + 1e-9 * abs(dmin) + 1e-300, name        # the minimum was found
        assert r["shift"] == nat["shift"], name                            # ... the natural order's
        # every group with a hypothesis inside the final threshold ran in FP64: none was left out by
        # a bound, by the screen, or by ending the symbol at the first column tile above the limit
        gmin = r["d"].reshape(4, 4, 16, 16, 16).min(axis=(1, 2, 4))        # [blk, kt]
        for blk, kt in zip(*np.nonzero(gmin <= dmin + thr)):
            assert (int(kt), int(blk)) in r["swept"], (name, kt, blk)
        for kt, blk in r["skipped"]:
            assert gmin[blk, kt] > dmin + thr, (name, kt, blk)


def test_fewer_fp64_groups_at_theta0(cases):
    dev = sum(r["fp64"] for name, a, r, nat in cases if name == "theta0")
    natural = sum(nat["fp64"] for name, a, r, nat in cases if name == "theta0")
    scr = sum(r["screen"] for name, a, r, nat in cases if name == "theta0")
    scr_nat = sum(nat["screen"] for name, a, r, nat in cases if name == "theta0")
    print(f"theta_0, 64 symbols: FP64 groups {natural} natural -> {dev} best-first; at the screen {scr_nat} -> {scr}")
    assert dev < natural
    # near the true channel (the converged regime) nothing is lost
    dev_n = sum(r["fp64"] for name, a, r, nat in cases if name == "near")
    nat_n = sum(nat["fp64"] for name, a, r, nat in cases if name == "near")
    assert dev_n <= nat_n
