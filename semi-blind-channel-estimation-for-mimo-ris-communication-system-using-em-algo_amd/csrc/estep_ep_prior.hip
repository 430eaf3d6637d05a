// Soft-input expectation-propagation E-step (sbce_estep_prior / sbce_em_prior with
// SBCE_ESTEP_EP): estep_ep_kernel's posterior moments with a-priori bit L-values
// EstepArgs::la [B][Td][NT][lgM] on the data symbols (ep_prior.h has the algorithm).  The moments
// are those of the a-posteriori pmf of the last pass, prior included, in the product form.
//
// Work split: estep_ep_kernel's -- one workgroup of 4 waves per 32 consecutive symbols of one
// trial, lin_stage_h once, 8 lanes per symbol with lane a = column a, G's column and conj(u_a) in
// registers across the passes.  Beside them the lane keeps the <= 6 sanitised L-values of its
// stream; the labels (64 int32) are the only addition to LDS.
// Pivot rule: a failed pivot in any pass gives the whole symbol the moments of its a-priori pmf
// and OR-s SBCE_STATUS_DETECTOR into the trial's status; a stream with mu_a <= 0 gets them for
// itself alone.  A workgroup whose trial is flagged in EstepArgs::done returns before staging.
// The moments are stored plainly (no moment-repeat fold).
// Determinism: every sum has an order fixed by (NT, NR, P, M, p) alone, cross-lane moves only
// copy, there is no floating-point atomic and no workgroup reads another's results: trial b of a
// B-trial call is bitwise the B = 1 call.
#include "ep_prior.h"

namespace sbce {

namespace {

struct EpPriorConst {
    int NR, P, Td, M, lgM, chunks;
    int passes;
    double varn;
};

template <int NT>
__global__ __launch_bounds__(kLinThreads, 3) void estep_ep_prior_kernel(EstepArgs a, EpPriorConst c) {
    __shared__ cd buf_s[kLinBuf];
    __shared__ cd cons_s[64];
    __shared__ int lab_s[64];
    __shared__ int fail_s;

    const int b = blockIdx.x / c.chunks, ch = blockIdx.x % c.chunks;
    if (a.done && a.done[b]) return;                    // block-uniform: a stopped trial

    const int NR = c.NR, P = c.P, Td = c.Td, M = c.M, lgM = c.lgM;
    const int NE = NT * NR;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = ch * kLinSym;
    const int tend = t0 + kLinSym < Td ? t0 + kLinSym : Td;
    const size_t bt = (size_t)b * Td;

    if (tid < M) {
        cons_s[tid] = a.cons[tid];
        lab_s[tid] = a.labels[tid];
    }
    if (tid == 0) fail_s = 0;

    lin_stage_h(buf_s, a.theta + (size_t)b * P * NE, a.psid + bt * P, NE, P, t0, tend);

    // 8 lanes per symbol, lane a = column a.  Lanes past NT and groups past the chunk repeat a
    // valid column (no divergence around the cross-lane moves) and store nothing.
    const int grp = lane >> 3, al = lane & 7;
    const int ts = t0 + w * 8 + grp;
    const bool act = al < NT && ts < tend;
    const int aa = al < NT ? al : 0;
    const int k = ts < tend ? w * 8 + grp : tend - 1 - t0;
    const size_t sym = bt + t0 + k;
    const double s2 = trial_noise(a.varn_t ? a.varn_t[b] : c.varn).s2;
    double es = 0.0;
    for (int s = 0; s < M; ++s) es += cabs2(cons_s[s]);
    es = uniform_d(es / (double)M);                     // every lane formed the same bits: to SGPRs

    const EpPrior pr = ep_prior_load(a.la + (sym * NT + aa) * lgM, lgM);
    cd c0[NT + 1];
    ep_gram<NT>(buf_s + k * kLinHS, a.yd + sym * NR, NR, aa, c0);
    cd t;
    double h2, inv;
    bool dead, fail;
    ep_prior_run<NT>(c0, cons_s, lab_s, M, lgM, pr, s2, es, c.passes, aa, lane, t, h2, inv, dead, fail);
    cd mean;
    double saa;
    ep_prior_demap(cons_s, lab_s, M, lgM, pr, t, inv, mean, saa);

    cd* mo = a.mom + sym * (NT + NT * NT);
    if (act) {
        mo[aa] = mean;
        if (fail) fail_s = 1;
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {   // uniform: the cross-lane moves see every lane
        const cd mq = bperm_c(mean, ((lane & 56) | q) << 2);
        if (act) mo[NT + aa * NT + q] = q == aa ? cmk(saa, 0.0) : cmulc(mean, mq);
    }
    __syncthreads();
    if (tid == 0 && fail_s && a.status) atomicOr(&a.status[b], SBCE_STATUS_DETECTOR);
}

template <int NT>
hipError_t launch_nt(const EstepArgs& a, const EpPriorConst& c, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(estep_ep_prior_kernel<NT>, dim3(blocks), dim3(kLinThreads), 0, s, a, c);
    return hipGetLastError();
}

}  // namespace

// EstepArgs::la and ::labels set; the limits are estep_ep_supported's
hipError_t launch_estep_ep_prior(const Problem& pb, const EstepArgs& a, hipStream_t s) {
    EpPriorConst c;
    c.NR = pb.NR; c.P = pb.P; c.Td = pb.Td; c.M = pb.M;
    c.lgM = 0;
    while ((1 << c.lgM) < pb.M) ++c.lgM;
    c.chunks = (pb.Td + kLinSym - 1) / kLinSym;
    c.passes = ep_passes_of(pb.pr);
    c.varn = pb.varn;
    const long long blocks = (long long)pb.B * c.chunks;
    if (blocks == 0) return hipSuccess;
    // the kernel's LDS buffers are sized for these limits: never launch past them
    if (!estep_ep_supported(pb) || !a.la || !a.labels) return hipErrorInvalidValue;
    switch (pb.NT) {
        case 1: return launch_nt<1>(a, c, (unsigned)blocks, s);
        case 2: return launch_nt<2>(a, c, (unsigned)blocks, s);
        case 3: return launch_nt<3>(a, c, (unsigned)blocks, s);
        case 4: return launch_nt<4>(a, c, (unsigned)blocks, s);
        case 5: return launch_nt<5>(a, c, (unsigned)blocks, s);
        case 6: return launch_nt<6>(a, c, (unsigned)blocks, s);
        case 7: return launch_nt<7>(a, c, (unsigned)blocks, s);
        case 8: return launch_nt<8>(a, c, (unsigned)blocks, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sbce
