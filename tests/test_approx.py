"""CPU tier of the Gaussian-approximation comparator EM ("Comparision/Comparision T_d vs
NMSE.py":106-145): the NumPy restatement the device kernel is checked against reproduces the
reference's own EM_approx on every fixture case, the signal-model replay reproduces the
comparison scripts' data, and the two new C-ABI entry points are exported, laid out as the
ctypes classes say and validate their arguments without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import approx_oracle as ao
from conftest import ROOT, golden, rel

N_SMALL = 6
SWEEP_TAGS = [("comparison_td", "td20"), ("comparison_td", "td100"),
              ("comparison_tp", "tp4"), ("comparison_tp", "tp40")]


def small_cases():
    d = golden("approx_small")
    for k in range(N_SMALL):
        n, m, tp, td, iters, varn = d["shapes"][k]
        yield k, {name: d[f"c{k}_{name}"] for name in ("Psi_p", "Psi_d", "x_p", "Y_p", "Y_d", "G0",
                                                        "G_hat")}, int(iters), float(varn)


def test_restatement_matches_reference_on_every_fixture_case():
    """G within 1e-10 relative of the reference's EM_approx (Iterations + 1 updates)."""
    worst = 0.0
    for k, c, iters, varn in small_cases():
        G = ao.em_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], iters + 1, varn)
        assert rel(ao.initial_g(c["Psi_p"], c["x_p"], c["Y_p"]), c["G0"]) < 1e-13, k
        e = rel(G, c["G_hat"])
        worst = max(worst, e)
        assert e < 1e-10, (k, e)
    for name, tag in SWEEP_TAGS:
        d = golden(name)
        G = ao.em_approx(d[f"{tag}_Psi_p"], d[f"{tag}_Psi_d"], d[f"{tag}_x_p"], d[f"{tag}_Y_p_dft"],
                         d[f"{tag}_Y_d_dft"], int(d["itera"]) + 1, float(d["varn"]))
        e = rel(G, d[f"{tag}_G_hat"])
        worst = max(worst, e)
        assert e < 1e-10, (tag, e)
    print(f"restatement vs reference, worst relative difference {worst:.2e}")


def test_restatement_tells_update_counts_and_hermitian_solves_apart():
    """The fixtures separate Iterations from Iterations + 1 updates, and a real-weight
    (Hermitian) normal matrix from the reference's complex one at varn = 1.0."""
    k, c, iters, varn = next(x for x in small_cases() if x[0] == 0)
    G3 = ao.em_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], iters, varn)
    assert rel(G3, c["G_hat"]) > 1e-6
    k, c, iters, varn = next(x for x in small_cases() if x[0] == 5)
    _, A, _, _ = ao.em_approx(c["Psi_p"], c["Psi_d"], c["x_p"], c["Y_p"], c["Y_d"], 1, varn,
                              first=True)
    assert np.linalg.norm(A - A.conj().T) / np.linalg.norm(A) > 1e-3


def _replay(sm, d, axis):
    """The comparison scripts' draw order through signal_model, one trial."""
    N, M, varn = int(d["N"]), int(d["n_rx"]), float(d["varn"])
    np.random.seed(int(d["seed"]))
    h, F_H, G, h_prop = sm.channel_matrix1(1.0, N, M, 1)
    out = dict(G=G, h_proposed=h_prop)
    if axis == "td":
        X_p = sm.pilot_symbols(1, 4, int(d["T_p"]))
    else:
        X_d, _ = sm.symbols(1, 4, int(d["T_d"]))
    for pt in d["T_d" if axis == "td" else "T_p"]:
        tp, td = (int(d["T_p"]), int(pt)) if axis == "td" else (int(pt), int(d["T_d"]))
        Ptp, Ptd = sm.irs_matrix_nodirect(tp, td, N)
        if axis == "td":
            X_d, _ = sm.symbols(1, 4, td)
        else:
            X_p = sm.pilot_symbols(1, 4, tp)
        x_p, x_d = np.vstack(X_p), np.vstack(X_d)
        Y_p, Y_d, U_p, _, _ = sm.received_signals(tp, td, Ptp, Ptd, M, 1, X_d, X_p, h_prop, varn,
                                                  with_initial=False)
        z_p, z_d = sm.noise_approx(varn, M, tp, td)
        Y_p_a, Y_d_a = sm.received_approx(h, F_H, Ptp, Ptd, x_d, x_p, z_p, z_d)
        tag = f"{axis}{int(pt)}"
        out.update({f"{tag}_Psi_p": Ptp, f"{tag}_Psi_d": Ptd, f"{tag}_Y_p": Y_p, f"{tag}_Y_d": Y_d,
                    f"{tag}_Y_p_dft": Y_p_a, f"{tag}_Y_d_dft": Y_d_a,
                    f"{tag}_G0": sm.initial_g_approx(Ptp, x_p, Y_p_a),
                    f"{tag}_h_init": sm.initial_estimate_per_pilot(U_p, Y_p, M)})
    return out


@pytest.mark.parametrize("name,axis", [("comparison_td", "td"), ("comparison_tp", "tp")])
def test_signal_model_replays_the_comparison_scripts(sbce, name, axis):
    """channel_matrix1, the no-direct phases, noise_approx and received_approx in the scripts'
    draw order reproduce the fixture's G, h_proposed, Psi_p, Psi_d, Y_p_dft, Y_d_dft and the
    proposed leg's Y_p, Y_d to <= 1e-15 relative."""
    d = golden(name)
    out = _replay(sbce.signal_model, d, axis)
    for key, val in out.items():
        if key.endswith("_G0") or key.endswith("_h_init"):
            continue
        e = rel(val, d[key])
        print(f"{name} {key}: {e:.2e}")
        assert val.shape == d[key].shape and e <= 1e-15, (key, e)
    # derived on the host from those (pseudo-inverses: rounding of an SVD, not a replay)
    for key, val in out.items():
        if key.endswith("_G0") or key.endswith("_h_init"):
            assert rel(val, d[key]) < 1e-12, key


def test_new_structs_match_c(sbce, tmp_path):
    """sizeof / offsetof of sbce_approx_dims and sbce_approx_ptrs (gcc) against the ctypes
    classes."""
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "sbce.h"
#define D(f) offsetof(sbce_approx_dims, f)
#define P(f) offsetof(sbce_approx_ptrs, f)
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sbce_approx_dims), D(batch), D(n_ris),
         D(n_rx), D(t_p), D(t_d), D(reserved), D(varn));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sbce_approx_ptrs), P(y_d), P(y_p),
         P(psi_d), P(psi_p), P(x_p), P(g), P(varn_t), P(status), P(workspace), P(workspace_bytes));
  printf("%d\n", SBCE_STATUS_SINGULAR);
  return 0;
}''')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    L = sbce._lib
    expect = ([ctypes.sizeof(L.ApproxDims)] + [getattr(L.ApproxDims, f).offset
                                               for f, _ in L.ApproxDims._fields_]
              + [ctypes.sizeof(L.ApproxPtrs)] + [getattr(L.ApproxPtrs, f).offset
                                                 for f, _ in L.ApproxPtrs._fields_]
              + [L.SBCE_STATUS_SINGULAR])
    assert [int(v) for v in out] == expect
    assert L.SBCE_STATUS_SINGULAR == 32


def _call(lib, L, dims, null_g=False, iters=3):
    buf = (ctypes.c_double * 64)()                       # 16-byte aligned host memory: validation
    a = ctypes.addressof(buf)                            # fails before any pointer is followed
    a += (-a) % 16
    ptrs = L.ApproxPtrs(a, a, a, a, a, None if null_g else a, None, None, None, 0)
    return lib.sbce_approx_em(ctypes.byref(dims), ctypes.byref(ptrs), iters, None)


@pytest.mark.parametrize("which", ["product", "ab"])
def test_validation_codes_without_gpu(sbce, which):
    L = sbce._lib
    lib = L.load() if which == "product" else L.load_ab()
    assert _call(lib, L, L.ApproxDims(4, 65, 8, 16, 20, 0, 0.1)) == -2       # N = 65
    assert _call(lib, L, L.ApproxDims(4, 32, 9, 16, 20, 0, 0.1)) == -2       # n_rx = 9
    assert _call(lib, L, L.ApproxDims(4, 32, 8, 16, 20, 0, 0.0)) == -1       # varn = 0
    assert _call(lib, L, L.ApproxDims(4, 32, 8, 16, 20, 0, 0.1), iters=0) == -1
    assert _call(lib, L, L.ApproxDims(4, 32, 8, 16, 20, 0, 0.1), null_g=True) == -1
    assert _call(lib, L, L.ApproxDims(0, 32, 8, 16, 20, 0, 0.1)) == -1       # batch < 1
    assert _call(lib, L, L.ApproxDims(4, 32, 8, 0, 20, 0, 0.1)) == -1        # t_p < 1
    assert _call(lib, L, L.ApproxDims(4, 32, 8, 16, 0, 0, 0.1)) == -1        # t_d < 1
    n = ctypes.c_size_t(7)
    d = L.ApproxDims(4, 32, 8, 16, 20, 0, 0.1)
    assert lib.sbce_approx_workspace_bytes(ctypes.byref(d), ctypes.byref(n)) == 0
    assert n.value == 0


def test_both_libraries_export_the_entry_points(sbce):
    L = sbce._lib
    for name in ("sbce_approx_workspace_bytes", "sbce_approx_em"):
        assert name in L.EXPORTED
        assert hasattr(L.load(), name) and hasattr(L.load_ab(), name)
    assert L.load().sbce_abi_version() == 7 and L.load_ab().sbce_abi_version() == 7
