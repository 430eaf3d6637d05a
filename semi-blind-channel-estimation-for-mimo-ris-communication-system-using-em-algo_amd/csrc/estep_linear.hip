// Soft ZF / MMSE E-step (SBCE_ESTEP_ZF_SOFT, SBCE_ESTEP_MMSE_SOFT): the posterior
// moments of per-stream linear equalisation with a Gaussian soft demapper, for n_tx up to 8.  Per
// (trial b, data symbol t), on the clean effective channel H = H_t (not the reference's
// off-by-one channel of the hard ZF / MMSE modes), with s2 = varn_b^2, es = mean |cons|^2,
// rho = s2 / es (MMSE) or 0 (ZF), A = H^H H + rho I = L L^H, g_a = (A^-1)_aa, z = A^-1 H^H y:
//   MMSE  mu_a = 1 - rho g_a,  x_soft_a = z_a / mu_a,  nu_a = s2 g_a / mu_a
//   ZF    x_soft_a = z_a,      nu_a = s2 g_a
//   post[a][s] ~ e^{-|x_soft_a - cons[s]|^2 / nu_a},  m_a = sum_s post cons,
//   S[a][a] = sum_s post |cons|^2,  S[a][c] = m_a conj(m_c)  (a product posterior).
// This is sbce_detect_linear's arithmetic (linear_solve.h: the same staging, Cholesky and estimate,
// operation for operation) without the detector's labels, bit-class minima, L-values, counters and
// zeroing kernel: one launch per E-step, one store (the moments).
//
// Work split: one workgroup of 4 waves per 32 consecutive symbols of one trial; theta and psi_d
// go through LDS in tiles of 32 rows of P; 8 lanes per symbol, lane a = column a of the augmented
// matrix (detect_linear.hip's header has the details).  The demapper of stream a is lane a's: one
// scan of the table for the minimum distance, one for the min-shifted sums (the nearest point has
// weight 1: nothing is 0 / 0).
// es is formed here from the table, by every lane, as one ascending-s sum: the host never reads
// cons.  A workgroup whose trial is flagged in EstepArgs::done returns before staging.
// Pivot rule: a pivot <= 1e-14 max_a A_aa gives the whole symbol the uniform posterior's moments
// and OR-s SBCE_STATUS_DETECTOR into the trial's status (NONHPD is the M-step's finding in the
// chain's status word); an MMSE stream with mu_a <= 0 gets the uniform posterior for itself alone.
// Determinism: every sum has an order fixed by (NT, NR, P, M) alone, cross-lane moves only copy,
// there is no floating-point atomic and no workgroup reads another's results: trial b of a B-trial
// call is bitwise the B = 1 call, and varn_t[b] == dims.varn gives the scalar call's bits
// (trial_noise).  The moments are stored plainly (no moment-repeat fold).
#include "linear_solve.h"

namespace sbce {

namespace {

struct LinEstepConst {
    int NR, P, Td, M, chunks;
    int mmse;
    double varn;
};

template <int NT>
__global__ __launch_bounds__(kLinThreads) void estep_linear_kernel(EstepArgs a, LinEstepConst c) {
    __shared__ cd buf_s[kLinBuf];
    __shared__ cd cons_s[64];
    __shared__ int fail_s;

    const int b = blockIdx.x / c.chunks, ch = blockIdx.x % c.chunks;
    if (a.done && a.done[b]) return;                    // block-uniform: a stopped trial

    const int NR = c.NR, P = c.P, Td = c.Td, M = c.M;
    const int NE = NT * NR;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = ch * kLinSym;
    const int tend = t0 + kLinSym < Td ? t0 + kLinSym : Td;
    const size_t bt = (size_t)b * Td;

    if (tid < M) cons_s[tid] = a.cons[tid];
    if (tid == 0) fail_s = 0;

    lin_stage_h(buf_s, a.theta + (size_t)b * P * NE, a.psid + bt * P, NE, P, t0, tend);

    // ---- solve: 8 lanes per symbol, lane a = column a.  Lanes past NT and groups past the chunk
    // repeat a valid column (no divergence around the cross-lane moves) and store nothing.
    const int grp = lane >> 3, al = lane & 7;
    const int ts = t0 + w * 8 + grp;
    const bool act = al < NT && ts < tend;
    const int aa = al < NT ? al : 0;
    const int k = ts < tend ? w * 8 + grp : tend - 1 - t0;
    const size_t sym = bt + t0 + k;
    const double s2 = trial_noise(a.varn_t ? a.varn_t[b] : c.varn).s2;
    double es = 0.0;
    for (int s = 0; s < M; ++s) es += cabs2(cons_s[s]);
    es /= (double)M;
    const bool mmse = c.mmse != 0;
    const double rho = mmse ? s2 / es : 0.0;

    double g;
    cd z;
    bool fail;
    lin_solve<NT>(buf_s + k * kLinHS, a.yd + sym * NR, NR, aa, lane, rho, g, z, fail);
    cd xs;
    double nu, inv;
    lin_estimate(mmse, rho, s2, g, z, fail, xs, nu, inv);

    // ---- demap of stream a
    double dmin = INFINITY;
    for (int s = 0; s < M; ++s) dmin = fmin(dmin, cabs2(csub(xs, cons_s[s])));
    double Z = 0.0, saa = 0.0;
    cd mean = czero();
    for (int s = 0; s < M; ++s) {
        const cd cs = cons_s[s];
        const double e = fexp_neg(-(cabs2(csub(xs, cs)) - dmin) * inv);
        Z += e;
        mean = caxpy(mean, e, cs);
        saa = fma(e, cabs2(cs), saa);
    }
    mean = cmk(mean.x / Z, mean.y / Z);
    saa /= Z;

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
hipError_t launch_nt(const EstepArgs& a, const LinEstepConst& c, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(estep_linear_kernel<NT>, dim3(blocks), dim3(kLinThreads), 0, s, a, c);
    return hipGetLastError();
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

hipError_t launch_estep_linear(const Problem& pb, const EstepArgs& a, int mode, hipStream_t s) {
    LinEstepConst c;
    c.NR = pb.NR; c.P = pb.P; c.Td = pb.Td; c.M = pb.M;
    c.chunks = (pb.Td + kLinSym - 1) / kLinSym;
    c.mmse = mode == SBCE_ESTEP_MMSE_SOFT;
    c.varn = pb.varn;
    const long long blocks = (long long)pb.B * c.chunks;
    if (blocks == 0) return hipSuccess;
    // the kernel's LDS buffers are sized for these limits: never launch past them
    if (!estep_linear_supported(pb, mode)) return hipErrorInvalidValue;
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
