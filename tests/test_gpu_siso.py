"""GPU tier of the soft-in / soft-out decoder (csrc/siso.hip; sbce_siso_decode) and of the
code-aided loop (em.turbo_em_batch): every output against the NumPy restatement of the header's
definition (tests/siso_oracle.py), the planted inputs, the bitwise properties (batch independence,
workspace contents, repetition, graph capture), the error codes through the loaded library, and
the loop stage by stage against the restated loop.

Bounds: lapp_u and le_c within C_k eps scale_t, scale_t the largest finite |A_t| of the step in the
oracle (at least 1) and C_k = 16 max(r_k, 1) with r_k measured on the CPU against a 50-digit copy
(siso_oracle.C_BY_OUTPUT); infinities equal exactly; u_hat and err exact outside the guarded bits
(|lapp_u| < 1e-6 scale_t; tests/test_siso.py asserts there are at most 1 % of them per case).
Nothing comes from the kernel."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

import prior_oracle as po
import siso_oracle as so

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
# (code, (batch, n_info, K, n, generators, flags)) of dims the library refuses (tests/test_siso.py
# runs the same list without a GPU)
BAD_DIMS = so.BAD_DIMS


def _check(got, o, code, perm, maxlog, B, what):
    """Every output of a B-codeword call against the first B codewords of the oracle's."""
    sc = so.scales(o, code, perm)
    worst = {}
    for k in ("lapp_u", "le_c"):
        g, w, s = got[k], o[k][:B], sc[k][:B]
        assert not np.isnan(g).any(), (what, k)
        inf = np.isinf(w)
        assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], w[inf]), (what, k)
        r = float((np.abs(g[~inf] - w[~inf]) / s[~inf]).max()) if (~inf).any() else 0.0
        worst[k] = r
        print(f"{what} {k}: {r:.3g} of C = {so.C_BY_OUTPUT[k + ('_maxlog' if maxlog else '')]:.3g}")
        assert r <= so.C_BY_OUTPUT[k + ("_maxlog" if maxlog else "")], (what, k, r)
    ok = ~so.guarded(o)[:B]
    assert np.array_equal(got["u_hat"][ok], o["u_hat"][:B][ok]), what
    return worst


@pytest.mark.parametrize("ci", range(len(so.CODES)))
def test_every_output_against_the_restatement(sbce, ci):
    """Every (n_info, termination, B, variant) of one code: parity of lapp_u, le_c, u_hat and err,
    and codeword b of the B-codeword call bitwise the B = 1 call's (b = 0) and the 17-call's."""
    K = so.CODES[ci][0]
    for n_info in so.n_info_list(K):
        for term in (True, False):
            c = so.case(ci, n_info, term)
            for variant in so.VARIANTS:
                lc, la, perm, maxlog = so.case_inputs(ci, n_info, term, variant)
                o = so.case_ref(ci, n_info, term, variant)
                runs = {}
                for B in so.batches(K):
                    what = f"code {ci} n_info {n_info} term {term} B {B} variant {variant}"
                    got = sbce.siso_decode_batch(lc[:B], c["code"], None if la is None else la[:B],
                                                 perm, u_true=c["u"][:B], maxlog=maxlog)
                    _check(got, o, c["code"], perm, maxlog, B, what)
                    ok = ~so.guarded(o)[:B]
                    want_err = (o["u_hat"][:B] != c["u"][:B])
                    if ok.all():
                        assert np.array_equal(got["err"], want_err.sum(axis=1)), what
                    else:
                        assert np.all(np.abs(got["err"] - want_err.sum(axis=1)) <= (~ok).sum(axis=1))
                    assert np.array_equal(got["err"], (got["u_hat"] != c["u"][:B]).sum(axis=1)), what
                    runs[B] = got
                big = runs[max(runs)]
                for B, got in runs.items():
                    for k in ("lapp_u", "le_c", "u_hat", "err"):
                        assert np.array_equal(got[k], big[k][:B]), (k, B, n_info, term, variant)


def _planted(ci, n_info, term):
    c = so.case(ci, n_info, term)
    lc, la = c["lc"][:5].copy(), c["la_u"][:5].copy()
    lc[0, 0], lc[0, 1], lc[0, 2], lc[0, 3] = np.nan, np.inf, -np.inf, 1e3
    la[0, 0], la[0, 1] = np.nan, -np.inf
    # codeword 1: the transmitted codeword known (+-inf), with the prior contradicting every bit
    sent = np.empty(lc.shape[1], dtype=int)
    sent[c["perm"]] = c["code"].encode(c["u"][1:2])[0]
    lc[1] = np.where(sent == 0, np.inf, -np.inf)
    la[1] = np.where(c["u"][1] == 0, -64.0, 64.0)
    # codeword 2: contradictory +-64 on the coded bits themselves (alternating, no codeword)
    lc[2] = 64.0 * (1 - 2 * (np.arange(lc.shape[1]) % 2))
    lc[3] = 0.0                                        # nothing known
    la[3] = 0.0
    lc[4] = -1e300                                     # every coded bit "1": clamped, no codeword
    return c, lc, la


@pytest.mark.parametrize("ci,n_info,term", [(0, 33, True), (4, 33, False), (5, 200, True)])
@pytest.mark.parametrize("maxlog", [False, True])
def test_planted_inputs_give_no_nan_and_inf_only_at_empty_classes(sbce, ci, n_info, term, maxlog):
    c, lc, la = _planted(ci, n_info, term)
    code, perm = c["code"], c["perm"]
    got = sbce.siso_decode_batch(lc, code, la, perm, maxlog=maxlog)
    o = so.siso_ref(lc, code, la, perm, maxlog)
    _check(got, o, code, perm, maxlog, 5, f"planted code {ci} maxlog {maxlog}")
    empty = so.empty_classes(code, n_info).reshape(-1)
    le = got["le_c"][:, perm]
    assert np.isfinite(got["lapp_u"]).all()
    assert np.array_equal(np.isposinf(le), np.broadcast_to(empty == 1, le.shape))
    assert np.array_equal(np.isneginf(le), np.broadcast_to(empty == -1, le.shape))
    assert np.array_equal(got["lapp_u"][3], np.zeros(n_info))      # nothing known: exact zeros
    # a known codeword alone (no contradicting prior) is returned
    alone = sbce.siso_decode_batch(lc[1:2], code, None, perm, maxlog=maxlog)
    assert np.array_equal(alone["u_hat"][0], c["u"][1])


def test_workspace_contents_repetition_and_graph_capture_leave_the_bits(sbce):
    """0x00- against 0xFF-filled workspace, the same call twice, and a captured call replayed into
    refilled outputs: the eager bits (K = 7 with a second wave of codewords, K = 4 packed)."""
    import torch
    for ci, n_info, term, B in ((5, 33, True, 3), (1, 200, False, 17)):
        c = so.case(ci, n_info, term)
        lc, la, perm = c["lc"][:B], c["la_u"][:B], c["perm"]
        runs = [sbce.siso_decode_batch(lc, c["code"], la, perm, u_true=c["u"][:B], ws_fill=f)
                for f in (0x00, 0xFF, 0x00)]
        for r in runs[1:]:
            for k, v in runs[0].items():
                assert np.array_equal(r[k], v), (k, ci)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (lc, la)]
        pm = torch.from_numpy(perm.copy()).cuda()
        ut = torch.from_numpy(np.ascontiguousarray(c["u"][:B], dtype=np.int32)).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = sbce.siso_decode_batch(dev[0], c["code"], dev[1], pm, u_true=ut,
                                         return_device=True)
        for _ in range(2):
            for v in out.values():
                v.fill_(1)
            g.replay()
            torch.cuda.synchronize()
            for k, v in runs[0].items():
                assert np.array_equal(out[k].cpu().numpy(), v), (k, ci)


def test_one_wave_arm_of_the_ab_build_gives_the_same_bits(sbce):
    """The A/B library's one-wave arm (alpha over every step, then beta with the outputs) against
    its two-wave kernel and the product's, odd and even n_steps: the same bits."""
    L = sbce._lib
    for ci, n_info, term, B in ((5, 33, True, 3), (5, 200, False, 2), (0, 33, True, 17),
                                (2, 2, False, 5)):
        c = so.case(ci, n_info, term)
        args = (c["lc"][:B], c["code"], c["la_u"][:B], c["perm"])
        prod = sbce.siso_decode_batch(*args, u_true=c["u"][:B])
        with L.debug_env() as ab:
            ab.sbce_debug_siso_onewave.restype = ctypes.c_int
            two = sbce.siso_decode_batch(*args, u_true=c["u"][:B])
            assert ab.sbce_debug_siso_onewave(1) == 0
            try:
                one = sbce.siso_decode_batch(*args, u_true=c["u"][:B], ws_fill=0xFF)
            finally:
                ab.sbce_debug_siso_onewave(0)
        for k, v in prod.items():
            assert np.array_equal(two[k], v) and np.array_equal(one[k], v), (k, ci, n_info)
    assert L.load().sbce_debug_siso_onewave(1) == EUNSUPPORTED     # the product has no switch


def _raw(sbce, B=2, n_info=5, K=3, n=2, gens=(7, 5, 0), flags=2):
    """Device buffers and the two structs of a small valid call."""
    import torch
    L = sbce._lib
    T = n_info + (K - 1 if flags & 2 else 0)
    dims = L.SisoDims(B, n_info, K, n, (ctypes.c_int32 * 3)(*gens), flags)
    t = dict(lc=torch.zeros(B * T * n + 2, dtype=torch.float64, device="cuda"),
             la=torch.zeros(B * n_info, dtype=torch.float64, device="cuda"),
             ut=torch.zeros(B * n_info, dtype=torch.int32, device="cuda"),
             lapp=torch.zeros(B * n_info, dtype=torch.float64, device="cuda"),
             err=torch.zeros(B, dtype=torch.int32, device="cuda"),
             ws=torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"))
    ptrs = L.SisoPtrs(t["lc"].data_ptr(), t["la"].data_ptr(), None, t["ut"].data_ptr(),
                      t["lapp"].data_ptr(), None, None, t["err"].data_ptr(), t["ws"].data_ptr(),
                      t["ws"].numel())
    return dims, ptrs, t


def test_error_codes_through_the_loaded_library(sbce):
    import torch
    L = sbce._lib
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    dims, ptrs, keep = _raw(sbce)
    assert lib.sbce_siso_decode(dims, ptrs, stream) == 0
    nb = ctypes.c_size_t(0)
    assert lib.sbce_siso_workspace_bytes(dims, ctypes.byref(nb)) == 0
    assert nb.value == 1 * 7 * 64 * 8                  # one group of 16 codewords, 7 steps
    ptrs.workspace_bytes = nb.value - 1
    assert lib.sbce_siso_decode(dims, ptrs, stream) == EWORKSPACE
    ptrs.workspace_bytes = nb.value
    assert lib.sbce_siso_decode(dims, ptrs, stream) == 0
    ptrs.lc += 4                                       # misaligned float64
    assert lib.sbce_siso_decode(dims, ptrs, stream) == EINVAL
    ptrs.lc += 4
    assert lib.sbce_siso_decode(dims, ptrs, stream) == 0
    # the checks of the dims come first: none of these reaches a launch, whatever the buffers
    for rc, (B, n_info, K, n, gens, flags) in BAD_DIMS:
        bad = L.SisoDims(B, n_info, K, n, (ctypes.c_int32 * 3)(*gens), flags)
        assert lib.sbce_siso_decode(bad, ptrs, stream) == rc, (B, n_info, K, n, gens, flags)
        assert lib.sbce_siso_workspace_bytes(bad, ctypes.byref(nb)) == rc
    ptrs.u_true = None                                 # err without u_true
    assert lib.sbce_siso_decode(dims, ptrs, stream) == EINVAL
    ptrs.err = None
    ptrs.lapp_u = None                                 # no output
    assert lib.sbce_siso_decode(dims, ptrs, stream) == EINVAL
    torch.cuda.synchronize()
    del keep


def test_turbo_loop_stage_by_stage_against_the_restated_loop(sbce):
    """Two outer iterations at the CPU tier's shape.  Each device stage is fed the restated loop's
    inputs and stays within its own existing bound -- the EM chain prior_oracle's per-trial bar,
    the detector prior_oracle's llr bound, the decoder this file's -- and the full device loop's
    u_hat equals the restated loop's outside guarded bits (equal bit errors where none is
    guarded)."""
    d = so.turbo_case()
    t = so.TURBO
    ref = so.turbo_ref(d, 2, t["itera"], t["passes"])
    B, T_d, n_tx = d["x_d"].shape
    args = (d["y_d"], d["y_p"], d["psi_d"], d["u_p"], d["cons"])
    theta_in = d["theta0"]
    for k, r in enumerate(ref):
        la_in = r["la_in"] if k else None
        th = sbce.em_batch(*args, r["sigma"], t["itera"], theta_in, mode="ep",
                           ep_passes=t["passes"], prior_llr=la_in, labels=d["labels"])["theta"]
        c = dict(d, varn=r["sigma"])
        for b in range(B):
            rr = po.chain(c, b, t["itera"], r["la_in"], theta0=theta_in[b], passes=t["passes"])
            pp = po.chain(c, b, t["itera"], r["la_in"], passes=t["passes"],
                          theta0=po.ep.perturbed(dict(theta0=theta_in), b))
            growth = max(np.linalg.norm(x - y) / np.linalg.norm(x)
                         for x, y in zip(rr["thetas"], pp["thetas"])) / po.ep.PERTURB
            bar = 64.0 * po.EPS * max(rr["kappa"], pp["kappa"]) * max(growth, 1.0)
            e = np.linalg.norm(th[b] - r["theta"][b]) / np.linalg.norm(r["theta"][b])
            print(f"outer {k} trial {b}: theta rel err {e:.3g}, bar {bar:.3g}")
            assert e <= bar, (k, b, e, bar)
        det = sbce.detect_linear_prior_batch(d["y_d"], d["psi_d"], d["cons"], r["theta"], d["varn"],
                                             n_tx, r["la_in"], kind=("ep", t["passes"]),
                                             labels=d["labels"], noise="true", want=("llr",))
        o = po.ep_prior_ref(d["y_d"], d["psi_d"], d["cons"], r["theta"], d["varn"], n_tx,
                            r["la_in"], passes=t["passes"], labels=d["labels"])
        rat = po.ratios(dict(llr=det["llr"]), o, d["cons"])
        print(f"outer {k}: detector llr ratio {rat['llr']:.3g} of {po.C_BY_OUTPUT['llr']:.3g}")
        assert rat["llr"] <= po.C_BY_OUTPUT["llr"]
        dec = sbce.siso_decode_batch(r["llr"], d["code"], perm=d["perm"])
        od = so.siso_ref(r["llr"], d["code"], None, d["perm"])
        _check(dec, od, d["code"], d["perm"], False, B, f"outer {k} decoder")
        theta_in = r["theta"]
    full = sbce.turbo_em_batch(*args, d["varn"], d["theta0"], n_tx, d["code"], d["perm"], outer=2,
                               itera=t["itera"], ep_passes=t["passes"], labels=d["labels"],
                               u_true=d["u"], h_true=d["h"])
    for k, (f, r) in enumerate(zip(full, ref)):
        ok = np.abs(r["lapp_u"]) >= so.GAP * r["scale"][:, :r["lapp_u"].shape[1]]
        assert np.array_equal(f["u_hat"][ok], r["u_hat"][ok]), k
        ber_dev, ber_ref = f["bit_errors"].sum(), (r["u_hat"] != d["u"]).sum()
        print(f"outer {k}: bit errors device {ber_dev} restated {ber_ref}, guarded {(~ok).sum()}, "
              f"NMSE {f['nmse'].mean():.4g}")
        if ok.all():
            assert ber_dev == ber_ref
