"""CPU tier of the soft-in / soft-out decoder (sbce_siso_decode) and the code-aided loop: what the
NumPy restatement (tests/siso_oracle.py) must satisfy whatever the kernel does -- it agrees with a
brute-force posterior over all codewords, puts its infinities exactly at the structurally empty
classes, returns zeros for zeros and the codeword for a known codeword -- the guard the GPU parity
tests (tests/test_gpu_siso.py) rely on, the bounds' constants against a 50-digit copy, the encoder,
qam.map_bits and synthetic_batch's x_d, the ABI's structs and argument checks, and the turbo loop
in NumPy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import crb_oracle as co
import siso_oracle as so

codec, qam = so.codec, so.qam


# ------------------------------------------------------------------ 1. the encoder
def test_encoder_known_answer_and_linearity():
    code = codec.ConvCode((0o7, 0o5), 3, True)
    assert code.encode(np.array([[1, 0, 1, 1]])).tolist() == [[1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1]]
    assert (code.n, code.n_steps(4), code.n_info_for(12)) == (2, 6, 4)
    for bad in (11, 4, 2):                             # odd; n_info = 0; n_info < 0
        with pytest.raises(ValueError):
            code.n_info_for(bad)
    rng = np.random.default_rng(3)
    for ci in range(len(so.CODES)):
        for term in (True, False):
            c = so.code_of(ci, term)
            a, b = rng.integers(0, 2, (2, 5, 23))
            assert np.array_equal(c.encode(a ^ b), c.encode(a) ^ c.encode(b))
            assert not c.encode(np.zeros((1, 23), dtype=int)).any()
            # the trellis of the oracle walks the same codeword
            nxt, cb = so.branch_tables(c)
            s, out = 0, []
            for u in list(a[0]) + [0] * (c.n_steps(23) - 23):
                out += list(cb[s, u])
                s = nxt[s, u]
            assert out == c.encode(a[:1])[0].tolist() and (s == 0 or not term)
    for gens, K in (((6, 5), 3), ((7, 3), 3), ((15, 5), 3), ((7,), 3), ((7, 5), 2), ((7, 5), 8)):
        with pytest.raises(ValueError):
            codec.ConvCode(gens, K)
    p = codec.random_interleaver(384, 5)
    assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(384))
    assert np.array_equal(p, codec.random_interleaver(384, 5))


def test_map_bits_inverts_bits_of_and_x_d_leaves_the_other_arrays(sbce):
    for M in (4, 16, 64):
        cons, labels = qam.qam_constellation(M), qam.gray_labeling(M)
        idx = np.random.default_rng(M).integers(0, M, (3, 5, 2))
        assert np.array_equal(qam.map_bits(qam.bits_of(labels)[idx], cons, labels), cons[idx])
    with pytest.raises(ValueError):
        qam.map_bits(np.zeros((3, 3), dtype=int), cons, labels)
    sm = sbce.signal_model
    a = sm.synthetic_batch(3, 2, 2, 3, 6, 5, 4, 0.1, seed=2)
    x = a["cons"][np.random.default_rng(0).integers(0, 4, a["x_d"].shape)]
    b = sm.synthetic_batch(3, 2, 2, 3, 6, 5, 4, 0.1, seed=2, x_d=x)
    for k in ("y_p", "psi_d", "u_p", "h", "theta0"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["x_d"], x) and not np.array_equal(a["y_d"], b["y_d"])
    H = np.einsum("btp,bpar->btra", b["psi_d"], b["h"].reshape(3, -1, 2, 2))
    noise_a = a["y_d"] - np.einsum("btra,bta->btr", H, a["x_d"])
    noise_b = b["y_d"] - np.einsum("btra,bta->btr", H, x)
    assert np.abs(noise_a - noise_b).max() < 1e-12     # the same noise draw


# ------------------------------------------------------------------ 2. restatement properties
@pytest.mark.parametrize("ci", range(len(so.CODES)))
def test_restatement_against_brute_force_and_empty_classes(ci):
    rng = np.random.default_rng(100 + ci)
    for term in (True, False):
        code = so.code_of(ci, term)
        for n_info in (1, 2, 7, 10):
            nc = code.n_steps(n_info) * code.n
            lc, la = rng.normal(0, 4, (2, nc)), rng.normal(0, 2, (2, n_info))
            lc[0, 0], la[1, 0] = np.inf, np.nan
            perm = codec.random_interleaver(nc, n_info)
            empty = so.empty_classes(code, n_info)
            for use_la, use_perm in ((True, True), (False, False)):
                o = so.siso_ref(lc, code, la if use_la else None, perm if use_perm else None)
                for b in range(2):
                    bf = so.brute_force(lc[b], code, la[b] if use_la else None,
                                        perm if use_perm else None)
                    for k in ("lapp_u", "le_c"):
                        x, y = o[k][b], bf[k]
                        inf = np.isinf(y)
                        assert not np.isnan(x).any()
                        assert np.array_equal(np.isinf(x), inf) and np.array_equal(x[inf], y[inf])
                        assert np.abs(x[~inf] - y[~inf]).max() < 1e-10, (ci, term, n_info, k)
                    le = o["le_c"][b][perm if use_perm else np.arange(nc)].reshape(-1, code.n)
                    sign = np.where(np.isposinf(le), 1, np.where(np.isneginf(le), -1, 0))
                    assert np.array_equal(sign, empty), (ci, term, n_info)
                    assert np.isfinite(o["lapp_u"]).all()
    # the header's example: g = (7, 5), n_info = 1, terminated: le_c[3] = +inf
    assert so.empty_classes(so.code_of(0, True), 1)[1, 1] == 1


def test_zero_input_and_known_codeword():
    for ci in (0, 4, 5):
        for term in (True, False):
            code = so.code_of(ci, term)
            for maxlog in (False, True):
                nc = code.n_steps(20) * code.n
                o = so.siso_ref(np.zeros((1, nc)), code, maxlog=maxlog)
                assert np.array_equal(o["lapp_u"], np.zeros((1, 20)))
                u = np.random.default_rng(ci).integers(0, 2, (3, 20))
                c = code.encode(u)
                o = so.siso_ref(np.where(c == 0, np.inf, -np.inf), code, maxlog=maxlog)
                assert np.array_equal(o["u_hat"], u)
                fin = np.isfinite(o["le_c"])
                assert np.array_equal(o["le_c"][fin] < 0, c[fin] == 1)


def test_guarded_share_of_the_gpu_cases():
    """At most 1 % of a case's bits have |lapp_u| below GAP x scale (the decisions the GPU tier
    does not compare), so u_hat and err are compared on at least 99 %."""
    worst = 0.0
    for cs in so.all_cases():
        g = so.guarded(so.case_ref(*cs))
        worst = max(worst, float(g.mean()))
        assert g.mean() <= 0.01, cs
    print(f"largest guarded share {worst:.4f}")
    d = so.turbo_case()
    for r in so.turbo_ref(d, 2, so.TURBO["itera"], so.TURBO["passes"]):
        assert (np.abs(r["lapp_u"]) < so.GAP * r["scale"][:, :r["lapp_u"].shape[1]]).mean() <= 0.01


def test_constants_against_extended_precision():
    """r_k of a subset of the parity cases (every code at n_info 33, the longest recursion of the
    smallest and the largest trellis) stays below the recorded R_BY_OUTPUT."""
    cases = [(ci, 33, ci % 2 == 0, so.VARIANTS[ci % 4]) for ci in range(len(so.CODES))]
    cases += [(0, 200, True, so.VARIANTS[1]), (5, 200, False, so.VARIANTS[0])]
    for k, (r, cs) in so.measure_constants(cases).items():
        print(f"{k}: r = {r:.3g} at {cs}")
        assert r <= so.R_BY_OUTPUT[k], (k, r, cs)
    assert so.C_BY_OUTPUT == {k: 16.0 * max(r, 1.0) for k, r in so.R_BY_OUTPUT.items()}


# ------------------------------------------------------------------ 3. the ABI
def test_struct_layout_matches_c(sbce, tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "sbce.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(sbce_siso_dims),
         offsetof(sbce_siso_dims, gen), offsetof(sbce_siso_dims, flags), sizeof(sbce_siso_ptrs),
         offsetof(sbce_siso_ptrs, u_true), offsetof(sbce_siso_ptrs, le_c),
         offsetof(sbce_siso_ptrs, workspace), offsetof(sbce_siso_ptrs, workspace_bytes),
         SBCE_SISO_TERMINATED);
  return 0;
}''')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    L = sbce._lib
    assert [int(v) for v in out] == [ctypes.sizeof(L.SisoDims), L.SisoDims.gen.offset,
                                     L.SisoDims.flags.offset, ctypes.sizeof(L.SisoPtrs),
                                     L.SisoPtrs.u_true.offset, L.SisoPtrs.le_c.offset,
                                     L.SisoPtrs.workspace.offset, L.SisoPtrs.workspace_bytes.offset,
                                     L.SBCE_SISO_TERMINATED]


def test_workspace_and_validation_without_gpu(sbce):
    """Every error code of sbce_siso_decode is decided before any HIP call: on a machine without a
    GPU the calls below return their codes (a launch would return SBCE_EHIP, -3)."""
    L = sbce._lib
    lib = L.load()
    nb = ctypes.c_size_t(0)

    def dims(B=5, n_info=33, K=7, n=2, gens=(0o133, 0o171, 0), flags=2):
        return L.SisoDims(B, n_info, K, n, (ctypes.c_int32 * 3)(*gens), flags)
    assert lib.sbce_siso_workspace_bytes(dims(), ctypes.byref(nb)) == 0
    assert nb.value == 5 * 39 * 64 * 8                 # S = 64: one codeword per group, 39 steps
    assert lib.sbce_siso_workspace_bytes(dims(B=17, K=3, gens=(7, 5, 0), flags=0),
                                         ctypes.byref(nb)) == 0
    assert nb.value == 2 * 33 * 64 * 8                 # S = 4: 16 codewords per group
    assert lib.sbce_siso_workspace_bytes(dims(), None) == -1
    assert lib.sbce_siso_workspace_bytes(None, ctypes.byref(nb)) == -1
    ok = lambda **kw: L.SisoPtrs(**{**dict(lc=256, lapp_u=256, workspace=256,
                                           workspace_bytes=1 << 40), **kw})
    for rc, (B, n_info, K, n, gens, flags) in so.BAD_DIMS:
        bad = dims(B, n_info, K, n, gens, flags)
        assert lib.sbce_siso_decode(bad, ok(), None) == rc, (B, n_info, K, n, gens, flags)
        assert lib.sbce_siso_workspace_bytes(bad, ctypes.byref(nb)) == rc
    d = dims()
    assert lib.sbce_siso_decode(None, ok(), None) == -1
    assert lib.sbce_siso_decode(d, None, None) == -1
    assert lib.sbce_siso_decode(d, ok(lc=None), None) == -1
    assert lib.sbce_siso_decode(d, ok(lapp_u=None), None) == -1            # no output
    assert lib.sbce_siso_decode(d, ok(err=256), None) == -1                # err without u_true
    assert lib.sbce_siso_decode(d, ok(workspace=None), None) == -1
    for f, v in (("lc", 260), ("la_u", 260), ("lapp_u", 260), ("le_c", 260), ("perm", 258),
                 ("u_true", 258), ("u_hat", 258), ("workspace", 264)):
        assert lib.sbce_siso_decode(d, ok(**{f: v}), None) == -1, f
    assert lib.sbce_siso_decode(d, ok(err=258, u_true=256), None) == -1
    assert lib.sbce_siso_decode(d, ok(workspace_bytes=5 * 39 * 64 * 8 - 1), None) == -4
    # K and n are judged before the generators, the generators before n_steps
    assert lib.sbce_siso_decode(dims(K=8, gens=(6, 5, 0)), ok(), None) == -2
    assert lib.sbce_siso_decode(dims(n_info=20000, gens=(6, 5, 0), K=3), ok(), None) == -1


def test_python_layer_has_no_cpu_path(sbce):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(sbce.SbceUnavailable):
            sbce.siso_decode_batch(np.zeros((1, 12)), codec.ConvCode((7, 5), 3))
    assert sbce.ConvCode is codec.ConvCode and sbce.random_interleaver is codec.random_interleaver


# ------------------------------------------------------------------ 4. the turbo loop in NumPy
def test_turbo_loop_gains_from_the_code():
    """4 x 4 streams, N = 3, 16-QAM, T_d = 24 (384 coded bits), g = (7, 5) terminated, a seeded
    interleaver: the bit errors after outer iteration 3 are fewer than after iteration 1, and the
    mean NMSE moves toward crb_oracle's genie bound without crossing it.  Only the ordering is
    asserted; the observed figures are in DESIGN.md section 3.16."""
    d, t = so.turbo_case(), so.TURBO
    ref = so.turbo_ref(d, t["outer"], t["itera"], t["passes"])
    B = t["B"]
    nrm = np.linalg.norm(d["h"], axis=1) ** 2
    genie = float(np.mean([co.crb_reduced(d["u_p"][b], d["psi_d"][b], co.genie_S(d["x_d"][b]),
                                          d["n_rx"], d["varn"])["mse"] / nrm[b] for b in range(B)]))
    nmse = [float(np.mean(np.linalg.norm(r["theta"] - d["h"], axis=1) ** 2 / nrm)) for r in ref]
    errs = [int((r["u_hat"] != d["u"]).sum()) for r in ref]
    print(f"bit errors {errs} of {d['u'].size}, NMSE {nmse}, genie bound {genie:.4g}")
    assert errs[2] < errs[0]
    assert genie < nmse[2] < nmse[0]
