// Linear soft detection (sbce_detect_linear): from a GIVEN channel estimate
// theta, for every (trial b, data symbol t), per-stream ZF / LMMSE equalisation with a Gaussian
// soft demapper.  With H = H_t the effective channel of sbce_detect, rho = sigma2 / es (MMSE) or
// 0 (ZF), A = H^H H + rho I = L L^H, g_a = (A^-1)_aa and z = A^-1 H^H y:
//   MMSE  mu_a = 1 - rho g_a,  x_soft_a = z_a / mu_a,  nu_a = es (1 - mu_a) / mu_a = sigma2 g_a / mu_a
//   ZF    x_soft_a = z_a,      nu_a = sigma2 g_a
// and each stream is demapped on its own: d_s = |x_soft_a - cons[s]|^2, weights e^{-d_s / nu_a}.
//
// Work split (the lane split, staging, solve, estimate and moment store are linear_solve.h's,
// shared with the E-steps of estep_linear.hip).  One workgroup of 4 waves takes 32 consecutive
// symbols of ONE trial.
//   staging  theta of the trial goes through LDS in tiles of 32 rows of P (32 x 64 x 16 B = 32 KB)
//            beside the tile's 32 x 32 phases of psi_d (16 KB), both by coalesced 16-byte loads.
//            Wave w forms H of its 8 symbols: lane = (entry e of the NE = NT NR, symbol subset g);
//            each sum over p is ONE ascending fma chain.  H then overwrites the staging buffers
//            (row stride 65: the symbols of a wave fall on different LDS slots).
//   solve    a group of 8 lanes per symbol (8 symbols per wave).  Lane a owns column a of the
//            augmented Hermitian matrix [A; (H^H y)^H] and runs a right-looking Cholesky: at
//            step j the pivot and the scaled column j come from lane j by ds_bpermute, every lane
//            a > j updates its column, and every lane advances its own forward substitution
//            L w = e_a with the same column.  Column j is dead after step j, so nothing is kept:
//            g_a = ||w||^2 and z_a = w^H u accumulate on the way (u = L^-1 H^H y is the augmented
//            row, broadcast with the column).  No back substitution, no division: pivots by
//            v_rsq_f64 + two Newton steps (fast_rsqrt64).
//   demap    lane a scans the table for stream a: minimum and per-bit-class minima, then the
//            min-shifted sums (the smallest member of every sum has weight 1: nothing is 0/0), the
//            posterior, its moments and the L-values.
// Pivot rule (the project's): a pivot <= 1e-14 max_a A_aa fails the whole symbol: x_soft = 0,
// nu = +inf, so the weights are all 1 (post = 1/M, llr = 0), and the trial gets NONHPD.
// Determinism: every sum has an order fixed by (NT, NR, P, M) alone, cross-lane moves only copy,
// the maximum and the integer counters are order-free, no floating-point atomic is used and no
// workgroup reads another's results: trial b of a B-trial call is bitwise the B = 1 call.
// Launches: one small kernel that zeroes err and status (when either is set), then the detection
// kernel: a linear chain of two kernel nodes on the caller's stream, no memset node.
//
// SBCE_LINEAR_EP (the EP instantiation of the kernel): the solve and the estimate are replaced by
// the passes of ep_solve.h on the same staged H, and x_soft = t, nu = h2 are the cavity mean and
// variance of the last pass; everything after them is the same code.
#include "ep_prior.h"

namespace sbce {

namespace {

// The LDS of a detection kernel
struct DetectLinearLds {
    cd buf[kLinBuf];
    cd cons[64];
    int lab[64];
    int cnt[3];        // symbol errors, bit errors, failed-pivot flag
};

// The head of both detection kernels: the table and the labels (the identity by default) to LDS,
// the counters to 0, H_t of the workgroup's symbols staged.  Out: the lane's work.
template <int NT>
__device__ __forceinline__ LinSplit detect_linear_head(const LinearArgs& a, DetectLinearLds& lds) {
    const LinSplit sp = lin_split(NT, a.Td, a.chunks);
    const int NE = NT * a.NR;
    lin_load_table(lds.cons, lds.lab, a.cons, a.labels, a.M);
    if (threadIdx.x < 3) lds.cnt[threadIdx.x] = 0;
    lin_stage_h(lds.buf, a.theta + (size_t)sp.b * a.P * NE, a.psid + sp.bt * a.P, NE, a.P, sp.t0,
                sp.tend);
    return sp;
}

// The tail of both detection kernels, after the demapper and its post and llr stores: the stream's
// estimate and decision, the error counts against x_d_true (nearest table point, ties to the
// lowest s), the failed-pivot flag, the moments, and the workgroup's adds to err and status.
template <int NT>
__device__ __forceinline__ void detect_linear_tail(const LinearArgs& a, DetectLinearLds& lds,
                                                   const LinSplit& sp, cd xs, double nu, int idx,
                                                   bool fail, cd mean, double saa) {
    const size_t o = sp.sym * NT + sp.aa;
    if (sp.act) {
        if (a.xsoft) a.xsoft[o] = xs;
        if (a.nu) a.nu[o] = nu;
        if (a.xhat) a.xhat[o] = lds.cons[idx];
        if (a.idx) a.idx[o] = idx;
        if (a.err) {
            const cd xt = a.xd[o];
            double bd = INFINITY;
            int bi = 0;
            for (int s = 0; s < a.M; ++s) {
                const double dx = cabs2(csub(lds.cons[s], xt));
                if (dx < bd) {
                    bd = dx;
                    bi = s;
                }
            }
            if (bi != idx) {
                atomicAdd(&lds.cnt[0], 1);
                atomicAdd(&lds.cnt[1], __popc((unsigned)(lds.lab[bi] ^ lds.lab[idx])));
            }
        }
        if (fail) lds.cnt[2] = 1;
    }
    if (a.mom) lin_store_moments<NT>(a.mom, sp, mean, saa);   // uniform: every lane calls it
    __syncthreads();
    if (threadIdx.x == 0) {
        if (a.err && (lds.cnt[0] | lds.cnt[1])) {
            atomicAdd(&a.err[2 * sp.b], lds.cnt[0]);
            atomicAdd(&a.err[2 * sp.b + 1], lds.cnt[1]);
        }
        if (a.status && lds.cnt[2]) atomicOr(&a.status[sp.b], SBCE_STATUS_NONHPD);
    }
}

template <int NT, bool EP>
__global__ __launch_bounds__(kLinThreads) void detect_linear_kernel(LinearArgs a) {
    __shared__ DetectLinearLds lds;
    const LinSplit sp = detect_linear_head<NT>(a, lds);
    const cd* cons_s = lds.cons;
    const int* lab_s = lds.lab;
    const int NR = a.NR, M = a.M, lgM = a.lgM;
    const int aa = sp.aa, lane = sp.lane;
    const size_t sym = sp.sym;

    // ---- solve: 8 lanes per symbol, lane a = column a
    const cd* Hs = lds.buf + sp.k * kLinHS;
    const double s2 = a.sigma2_t ? a.sigma2_t[sp.b] : a.sigma2;
    const bool mmse = a.kind == SBCE_LINEAR_MMSE;
    const double rho = mmse ? s2 / a.es : 0.0;

    double g;
    cd z;
    bool fail;
    if constexpr (!EP) lin_solve<NT>(Hs, a.yd + sym * NR, NR, aa, lane, rho, g, z, fail);
    cd xs;
    double nu, inv;
    if constexpr (!EP) {
        lin_estimate(mmse, rho, s2, g, z, fail, xs, nu, inv);
    } else {
        cd c0[NT + 1];
        ep_gram<NT>(Hs, a.yd + sym * NR, NR, aa, c0);
        ep_run<NT>(c0, cons_s, M, s2, a.es, a.passes, aa, lane, xs, nu, inv, fail);
    }

    // ---- demap of stream a
    double dmin = INFINITY;
    int idx = 0;
    double m0[6], m1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m0[i] = m1[i] = INFINITY;
    for (int s = 0; s < M; ++s) {
        const double d = cabs2(csub(xs, cons_s[s]));
        if (d < dmin) {
            dmin = d;
            idx = s;
        }
        const int lb = lab_s[s];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const bool one = (lb >> i) & 1;
            m0[i] = one ? m0[i] : fmin(m0[i], d);
            m1[i] = one ? fmin(m1[i], d) : m1[i];
        }
    }
    double Z = 0.0, saa = 0.0;
    cd mean = czero();
    double T0[6], T1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) T0[i] = T1[i] = 0.0;
    for (int s = 0; s < M; ++s) {
        const cd cs = cons_s[s];
        const double d = cabs2(csub(xs, cs));
        const double e = fexp_neg(-(d - dmin) * inv);
        Z += e;
        mean = caxpy(mean, e, cs);
        saa = fma(e, cabs2(cs), saa);
        if (a.llr && !a.maxlog) {
            const int lb = lab_s[s];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                if (i < lgM) {
                    const bool one = (lb >> i) & 1;
                    const double ec = fexp_neg(-(d - (one ? m1[i] : m0[i])) * inv);
                    T0[i] = one ? T0[i] : T0[i] + ec;
                    T1[i] = one ? T1[i] + ec : T1[i];
                }
            }
        }
    }
    mean = cmk(mean.x / Z, mean.y / Z);
    saa /= Z;

    if (sp.act) {
        const size_t o = sym * NT + aa;
        if (a.post)
            for (int s = 0; s < M; ++s) {
                const double d = cabs2(csub(xs, cons_s[s]));
                a.post[o * M + s] = fexp_neg(-(d - dmin) * inv) / Z;
            }
        if (a.llr) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (i < lgM) {
                    double l = (m1[i] - m0[i]) * inv;
                    if (!a.maxlog) l += log(T0[i]) - log(T1[i]);
                    a.llr[o * lgM + i] = l;
                }
        }
    }
    detect_linear_tail<NT>(a, lds, sp, xs, nu, idx, fail, mean, saa);
}

// sbce_detect_linear_prior: the EP instantiation above with a-priori bit L-values
// la [B][Td][NT][lgM] -- the passes start from the prior's moments and every demapper weight
// carries the point's a-priori probability (ep_prior.h).  x_soft = t and nu = h2 are the extrinsic
// estimate of the last pass; post, the moments and the decision are a-posteriori (exponent
// -d_s / h2 + lp[s], the decision its argmax with ties to the lowest s); llr = L_post - La is
// extrinsic.  A dead stream (failed symbol, or mu <= 0) has x_soft = 0, nu = +inf, post = the
// a-priori pmf and llr = 0.
template <int NT>
__global__ __launch_bounds__(kLinThreads, 3) void detect_linear_prior_kernel(LinearArgs a,
                                                                             const double* la) {
    __shared__ DetectLinearLds lds;
    const LinSplit sp = detect_linear_head<NT>(a, lds);
    const cd* cons_s = lds.cons;
    const int* lab_s = lds.lab;
    const int NR = a.NR, M = a.M, lgM = a.lgM;
    const int aa = sp.aa, lane = sp.lane;
    const size_t sym = sp.sym;
    const double s2 = a.sigma2_t ? a.sigma2_t[sp.b] : a.sigma2;
    const size_t o = sym * NT + aa;

    const EpPrior pr = ep_prior_load(la + o * lgM, lgM);
    cd xs;
    double nu, inv;
    bool dead, fail;
    {
        cd c0[NT + 1];
        ep_gram<NT>(lds.buf + sp.k * kLinHS, a.yd + sym * NR, NR, aa, c0);
        ep_prior_run<NT>(c0, cons_s, lab_s, M, lgM, pr, s2, a.es, a.passes, aa, lane, xs, nu, inv,
                         dead, fail);
    }

    // ---- demap of stream a: the largest exponent, its index and the per-bit-class maxima, then
    // the max-shifted sums (the largest member of every sum has weight 1: nothing is 0/0)
    double emax = -INFINITY;
    int idx = 0;
    double m0[6], m1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m0[i] = m1[i] = -INFINITY;
    for (int s = 0; s < M; ++s) {
        const int lb = lab_s[s];
        const double e = ep_prior_exponent(pr, cons_s[s], lb, lgM, xs, inv);
        if (e > emax) {
            emax = e;
            idx = s;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const bool one = (lb >> i) & 1;
            m0[i] = one ? m0[i] : fmax(m0[i], e);
            m1[i] = one ? fmax(m1[i], e) : m1[i];
        }
    }
    double Z = 0.0, saa = 0.0;
    cd mean = czero();
    double T0[6], T1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) T0[i] = T1[i] = 0.0;
    for (int s = 0; s < M; ++s) {
        const cd cs = cons_s[s];
        const int lb = lab_s[s];
        const double ex = ep_prior_exponent(pr, cs, lb, lgM, xs, inv);
        const double e = fexp_neg(ex - emax);
        Z += e;
        mean = caxpy(mean, e, cs);
        saa = fma(e, cabs2(cs), saa);
        if (a.llr && !a.maxlog) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                if (i < lgM) {
                    const bool one = (lb >> i) & 1;
                    const double ec = fexp_neg(ex - (one ? m1[i] : m0[i]));
                    T0[i] = one ? T0[i] : T0[i] + ec;
                    T1[i] = one ? T1[i] + ec : T1[i];
                }
            }
        }
    }
    mean = cmk(mean.x / Z, mean.y / Z);
    saa /= Z;

    if (sp.act) {
        if (a.post)
            for (int s = 0; s < M; ++s)
                a.post[o * M + s] =
                    fexp_neg(ep_prior_exponent(pr, cons_s[s], lab_s[s], lgM, xs, inv) - emax) / Z;
        if (a.llr) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (i < lgM) {
                    double l = m0[i] - m1[i];
                    if (!a.maxlog) l += log(T0[i]) - log(T1[i]);
                    a.llr[o * lgM + i] = dead ? 0.0 : l - ep_prior_la(pr, i);
                }
        }
    }
    detect_linear_tail<NT>(a, lds, sp, xs, nu, idx, fail, mean, saa);
}

// err[b][0..1] = 0 and status[b] = 0 (each when set) ahead of the detection kernel's integer adds
// and ORs.  A kernel, not hipMemsetAsync: in the graph-capture test the memset nodes of this call
// were observed to leave stale words in err and status on replay (HIP 7.0 runtime; the cause is
// not established); kernel nodes replayed as captured.
__global__ __launch_bounds__(256) void linear_zero_kernel(int32_t* err, int32_t* status, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (err && i < 2 * B) err[i] = 0;
    if (status && i < B) status[i] = 0;
}

}  // namespace

bool detect_linear_supported(int NT, int NR) { return NT >= 1 && NT <= 8 && NR >= 1 && NR <= 8; }

hipError_t launch_detect_linear(LinearArgs a, hipStream_t s) {
    return launch_detect_linear_prior(a, nullptr, s);
}

hipError_t launch_detect_linear_prior(LinearArgs a, const double* la, hipStream_t s) {
    if (la && (a.kind != SBCE_LINEAR_EP || !a.labels)) return hipErrorInvalidValue;
    a.lgM = 0;
    while ((1 << a.lgM) < a.M) ++a.lgM;
    a.chunks = (a.Td + kLinSym - 1) / kLinSym;
    if ((long long)a.B * a.chunks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.err || a.status) {
        hipLaunchKernelGGL(linear_zero_kernel, dim3((unsigned)((2LL * a.B + 255) / 256)), dim3(256), 0,
                           s, a.err, a.status, a.B);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return lin_dispatch_nt(a.NT, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        const dim3 grid((unsigned)(a.B * a.chunks)), block(kLinThreads);
        if (la)
            hipLaunchKernelGGL(detect_linear_prior_kernel<NT>, grid, block, 0, s, a, la);
        else if (a.kind == SBCE_LINEAR_EP)
            hipLaunchKernelGGL((detect_linear_kernel<NT, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((detect_linear_kernel<NT, false>), grid, block, 0, s, a);
        return hipGetLastError();
    });
}

}  // namespace sbce
