// The E-steps of the linear family, for n_tx up to 8: soft ZF / MMSE (SBCE_ESTEP_ZF_SOFT,
// SBCE_ESTEP_MMSE_SOFT), expectation propagation (SBCE_ESTEP_EP; §3.13) and EP
// with a-priori bit L-values (sbce_estep_prior / sbce_em_prior; §3.15).  One kernel template over
// n_tx and the kind; the kinds differ in the labels they keep, the L-value load, the solve and the
// last demapper, and share everything around them.  Per (trial b, data symbol t), on the clean
// effective channel H = H_t (not the reference's off-by-one channel of the hard ZF / MMSE modes),
// with s2 = varn_b^2 and es = mean |cons|^2:
//   ZF / MMSE  rho = s2 / es (MMSE) or 0 (ZF), A = H^H H + rho I = L L^H, g_a = (A^-1)_aa,
//              z = A^-1 H^H y:
//                MMSE  mu_a = 1 - rho g_a,  x_soft_a = z_a / mu_a,  nu_a = s2 g_a / mu_a
//                ZF    x_soft_a = z_a,      nu_a = s2 g_a
//              This is sbce_detect_linear's arithmetic (linear_solve.h: the same staging, Cholesky
//              and estimate, operation for operation).
//   EP         p passes of ep_solve.h; (x_soft, nu) = the cavity (t, h2) of the last pass.  Pass 1
//              is the soft MMSE solve; every further pass repeats it with the demapper's
//              per-stream means and variances as the prior.  G's column and conj(u_a) are read
//              from LDS once (ep_gram) and the passes run on registers.
//   EP, prior  the same with EstepArgs::la [B][Td][NT][lgM] (ep_prior.h): the passes start from
//              the a-priori pmf's moments and every demapper weight carries the point's a-priori
//              probability.  Beside G's column the lane keeps the <= 6 sanitised L-values of its
//              stream; the labels (64 int32) are the only addition to LDS.
//   post[a][s] ~ e^{-|x_soft_a - cons[s]|^2 / nu_a} (times the prior),  m_a = sum_s post cons,
//   S[a][a] = sum_s post |cons|^2,  S[a][c] = m_a conj(m_c)  (a product posterior).
// One launch per E-step, one store (the moments).
//
// Work split: one workgroup of 4 waves per 32 consecutive symbols of one trial; theta and psi_d
// go through LDS in tiles of 32 rows of P; 8 lanes per symbol, lane a = column a of the augmented
// matrix (detect_linear.hip's header has the details).  The demapper of stream a is lane a's.
// es is formed here from the table, by every lane, as one ascending-s sum: the host never reads
// cons.  A workgroup whose trial is flagged in EstepArgs::done returns before staging.
// Pivot rule: a pivot <= 1e-14 max_a A_aa (in any pass) gives the whole symbol the moments of the
// uniform posterior (prior kind: of its a-priori pmf) and OR-s SBCE_STATUS_DETECTOR into the
// trial's status (NONHPD is the M-step's finding in the chain's status word); an MMSE or EP stream
// with mu_a <= 0 gets them for itself alone.
// Determinism: every sum has an order fixed by (NT, NR, P, M, p) alone, cross-lane moves only
// copy, there is no floating-point atomic and no workgroup reads another's results: trial b of a
// B-trial call is bitwise the B = 1 call, and varn_t[b] == dims.varn gives the scalar call's bits
// (trial_noise).  The moments are stored plainly (no moment-repeat fold).
#include "ep_prior.h"

namespace sbce {

namespace {

enum LinEstepKind { kLinSoft, kLinEp, kLinEpPrior };

struct LinEstepConst {
    int NR, P, Td, M, lgM, chunks;
    int mmse;          // kLinSoft: MMSE, not ZF
    int passes;        // the EP kinds
    double varn;
};

template <int NT, int KIND>
__device__ __forceinline__ void estep_linear_body(const EstepArgs& a, const LinEstepConst& c) {
    constexpr bool kPrior = KIND == kLinEpPrior;
    __shared__ cd buf_s[kLinBuf];
    __shared__ cd cons_s[64];
    __shared__ int lab_s[64];       // the prior kind's; no other kind refers to it
    __shared__ int fail_s;

    const LinSplit sp = lin_split(NT, c.Td, c.chunks);
    if (a.done && a.done[sp.b]) return;                 // block-uniform: a stopped trial

    const int NR = c.NR, P = c.P, M = c.M;
    const int NE = NT * NR;
    lin_load_table(cons_s, kPrior ? lab_s : nullptr, a.cons, a.labels, M);
    if (threadIdx.x == 0) fail_s = 0;

    lin_stage_h(buf_s, a.theta + (size_t)sp.b * P * NE, a.psid + sp.bt * P, NE, P, sp.t0, sp.tend);

    const double s2 = trial_noise(a.varn_t ? a.varn_t[sp.b] : c.varn).s2;
    const cd* Hs = buf_s + sp.k * kLinHS;
    const cd* y = a.yd + sp.sym * NR;
    cd xs, mean;
    double nu, inv, saa;
    bool fail;
    if constexpr (KIND == kLinSoft) {
        const double es = lin_table_energy(cons_s, M);
        const bool mmse = c.mmse != 0;
        const double rho = mmse ? s2 / es : 0.0;
        double g;
        cd z;
        lin_solve<NT>(Hs, y, NR, sp.aa, sp.lane, rho, g, z, fail);
        lin_estimate(mmse, rho, s2, g, z, fail, xs, nu, inv);
        lin_demap(cons_s, M, xs, inv, mean, saa);
    } else {
        // every lane forms the same bits: to SGPRs
        const double es = uniform_d(lin_table_energy(cons_s, M));
        cd c0[NT + 1];
        if constexpr (kPrior) {
            const int lgM = c.lgM;
            const EpPrior pr = ep_prior_load(a.la + (sp.sym * NT + sp.aa) * lgM, lgM);
            ep_gram<NT>(Hs, y, NR, sp.aa, c0);
            bool dead;
            ep_prior_run<NT>(c0, cons_s, lab_s, M, lgM, pr, s2, es, c.passes, sp.aa, sp.lane, xs,
                             nu, inv, dead, fail);
            ep_prior_demap(cons_s, lab_s, M, lgM, pr, xs, inv, mean, saa);
        } else {
            ep_gram<NT>(Hs, y, NR, sp.aa, c0);
            ep_run<NT>(c0, cons_s, M, s2, es, c.passes, sp.aa, sp.lane, xs, nu, inv, fail);
            lin_demap(cons_s, M, xs, inv, mean, saa);
        }
    }

    if (sp.act && fail) fail_s = 1;
    lin_store_moments<NT>(a.mom, sp, mean, saa);
    __syncthreads();
    if (threadIdx.x == 0 && fail_s && a.status) atomicOr(&a.status[sp.b], SBCE_STATUS_DETECTOR);
}

// The soft ZF / MMSE kind has no minimum-waves bound; the EP kinds ask for 3 waves per SIMD.
template <int NT>
__global__ __launch_bounds__(kLinThreads) void estep_linear_kernel(EstepArgs a, LinEstepConst c) {
    estep_linear_body<NT, kLinSoft>(a, c);
}

template <int NT, int KIND>
__global__ __launch_bounds__(kLinThreads, 3) void estep_ep_kernel(EstepArgs a, LinEstepConst c) {
    estep_linear_body<NT, KIND>(a, c);
}

}  // namespace

bool estep_linear_mode(int mode) {
    return mode == SBCE_ESTEP_MMSE_SOFT || mode == SBCE_ESTEP_ZF_SOFT;
}

bool estep_linear_supported(const Problem& pb, int mode) {
    if (pb.NT < 1 || pb.NT > 8 || pb.NR < 1 || pb.NR > 8) return false;
    if (pb.M < 2 || pb.M > 64 || (pb.M & (pb.M - 1))) return false;
    if ((long long)pb.B * ((pb.Td + kLinSym - 1) / kLinSym) > 0x7fffffffLL) return false;
    return mode == SBCE_ESTEP_MMSE_SOFT || pb.NR >= pb.NT;   // ZF: A = H^H H needs n_rx >= n_tx
}

// SBCE_ESTEP_EP's limits are the soft MMSE E-step's, and partition_r carries the pass count
bool estep_ep_supported(const Problem& pb) {
    return estep_linear_supported(pb, SBCE_ESTEP_MMSE_SOFT) && ep_passes_of(pb.pr) > 0;
}

hipError_t launch_estep_linear(const Problem& pb, const EstepArgs& a, int mode, hipStream_t s) {
    const bool ep = mode == SBCE_ESTEP_EP;
    LinEstepConst c;
    c.NR = pb.NR; c.P = pb.P; c.Td = pb.Td; c.M = pb.M;
    c.lgM = 0;
    while ((1 << c.lgM) < pb.M) ++c.lgM;
    c.chunks = (pb.Td + kLinSym - 1) / kLinSym;
    c.mmse = mode == SBCE_ESTEP_MMSE_SOFT;
    c.passes = ep ? ep_passes_of(pb.pr) : 0;
    c.varn = pb.varn;
    const long long blocks = (long long)pb.B * c.chunks;
    if (blocks == 0) return hipSuccess;
    // the kernel's LDS buffers are sized for these limits: never launch past them
    const bool ok = ep ? estep_ep_supported(pb) && (!a.la || a.labels)
                       : estep_linear_supported(pb, mode);
    if (!ok) return hipErrorInvalidValue;
    return lin_dispatch_nt(pb.NT, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        const dim3 grid((unsigned)blocks), block(kLinThreads);
        if (!ep)
            hipLaunchKernelGGL(estep_linear_kernel<NT>, grid, block, 0, s, a, c);
        else if (a.la)
            hipLaunchKernelGGL((estep_ep_kernel<NT, kLinEpPrior>), grid, block, 0, s, a, c);
        else
            hipLaunchKernelGGL((estep_ep_kernel<NT, kLinEp>), grid, block, 0, s, a, c);
        return hipGetLastError();
    });
}

}  // namespace sbce
