// Batched data detector and soft demapper (sbce_detect): from a GIVEN channel
// estimate theta, for every (trial b, data symbol t), the joint decision, the per-stream symbol
// posteriors and the bit L-values over all J = M^NT hypotheses x_j (itertools.product order,
// first stream slowest), d_j = ||y_t - H_t x_j||^2.  The L-value is log(p0 / p1) of
// "Proposed method/QAM.py":164-185 on the MIMO posterior; cons is any table, labels any
// permutation (no grid structure is used anywhere).
//
// Work split, effective channels H_t and the distance arithmetic: hyp_enum.h (shared with
// loglik.hip).  One workgroup of 4 waves takes TC consecutive symbols of ONE trial, then ONE WAVE
// PER SYMBOL: lane l owns the prefix rows q = 64 qb + l and loops over the last stream s.
//
// Log-domain scheme.  The quantities wanted are sums of e^{-d_j/s2} over the classes
// C(a, v) = {j : x_j[a] = cons[v]} (NT M classes; bit sums are unions of M/2 classes).  A global
// shift would underflow a whole class at |LLR| ~ 1e6, so every class carries its OWN minimum:
//   pass 1  distances; class minima cmin[a][v] (exact, order-free: wave min for the last
//           stream, integer LDS atomic min on the bit pattern of d >= 0 for the others) and the
//           joint argmin (strict <, so ties go to the lowest j)
//   pass 2  distances again; the last stream's class sums  sum e^{-(d - cmin[NT-1][s])/s2}  by
//           a wave sum per (qb, s); per row an online log-sum-exp pair (rm, rS) over s, which
//           enters class (a, digit_a(q)) as rS e^{-(rm - cmin)/s2}: a butterfly over the lane
//           bits outside the digit adds the rows of a block that share the digit
//   final   post[a][s] = S e^{-(cmin - m*)/s2} / Z_a;  llr[a][i] = (m1 - m0)/s2 + log T0 - log T1
//           with m_v, T_v the minimum and the min-shifted sum over the classes whose label has
//           bit i = v.  The smallest member of every sum has weight 1: nothing is 0/0 or inf.
// Every reduction (DPP wave sums, butterflies, the qb loop) has an order fixed by the shape, no
// floating-point atomic is used and nothing is shared between workgroups: trial b of a B-trial
// call gives bitwise the result of a B = 1 call.  The error counters are integer atomic adds.
#include "hyp_enum.h"

namespace sbce {

namespace {

constexpr int kMaxCls = 128;        // NT * M (M^NT <= 65536)

__device__ __forceinline__ unsigned long long dbits(double v) {
    return (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ double bitsd(unsigned long long v) {
    return __longlong_as_double((long long)v);
}

template <int NRP>
__global__ __launch_bounds__(kHypThreads) void detect_kernel(DetectArgs a) {
    __shared__ cd th_s[kHypPT * kHypMaxNE];
    __shared__ cd cons_s[64];
    __shared__ int lab_s[64];
    __shared__ cd H_s[kHypWaves][kHypMaxSym][kHypMaxNE];
    __shared__ unsigned long long cmin_s[kHypWaves][kMaxCls];
    __shared__ double csum_s[kHypWaves][kMaxCls];

    const int NT = a.NT, NR = a.NR, P = a.P, Td = a.Td, M = a.M, lgM = a.lgM;
    const int NE = NT * NR;
    const int b = blockIdx.x / a.chunks, ch = blockIdx.x % a.chunks;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = ch * a.TC;
    const int tend = t0 + a.TC < Td ? t0 + a.TC : Td;
    const size_t bt = (size_t)b * Td;

    if (tid < M) {
        cons_s[tid] = a.cons[tid];
        lab_s[tid] = a.labels ? a.labels[tid] : tid;
    }

    heff_stage(H_s, th_s, a.theta, a.psid, b, bt, P, NE, t0, tend, tid, lane, w);
    __syncthreads();

    const int Q = 1 << (lgM * (NT - 1));
    const int nqb = (Q + 63) >> 6;
    const int ncls = NT * M;
    const int last = (NT - 1) * M;
    const double s2 = a.sigma2_t ? a.sigma2_t[b] : a.sigma2;
    const double inv = 1.0 / s2;
    unsigned long long* cmin = cmin_s[w];
    double* csum = csum_s[w];
    int nse = 0, nbe = 0;

    for (int k = 0; k < kHypMaxSym; ++k) {
        const int t = t0 + w + kHypWaves * k;
        if (t >= tend) break;                       // wave-uniform
        const cd* Hw = H_s[w][k];
        cd yv[NRP], hl[NRP];
#pragma unroll
        for (int i = 0; i < NRP; ++i) {
            const int ic = i < NR ? i : 0;
            yv[i] = csel(i < NR, a.yd[(bt + t) * NR + ic], czero());
            hl[i] = csel(i < NR, Hw[(NT - 1) * NR + ic], czero());
        }
        for (int i = lane; i < ncls; i += 64) {
            cmin[i] = dbits(INFINITY);
            csum[i] = 0.0;
        }
        wave_sync();

        // ---- pass 1: class minima and the joint argmin
        double bestd = INFINITY;
        int bestj = 0x7fffffff;
        for (int qb = 0; qb < nqb; ++qb) {
            const int q = (qb << 6) + lane;
            const bool valid = q < Q;
            cd rr[NRP];
            residual<NRP>(rr, yv, Hw, cons_s, q, NT, NR, lgM, M);
            double rowmin = INFINITY;
            for (int s = 0; s < M; ++s) {
                const double d = dist2<NRP>(rr, hl, cons_s[s]);
                const double dd = valid ? d : INFINITY;
                if (dd < bestd) {
                    bestd = dd;
                    bestj = q * M + s;
                }
                rowmin = fmin(rowmin, dd);
                const unsigned long long cm = dbits(wave_min_dpp(dd));
                if (lane == 0 && cm < cmin[last + s]) cmin[last + s] = cm;
            }
            if (valid)
                for (int x = 0; x < NT - 1; ++x)
                    atomicMin(&cmin[x * M + ((q >> (lgM * (NT - 2 - x))) & (M - 1))], dbits(rowmin));
        }
        wave_argmin_dpp(bestd, bestj);
        wave_sync();

        // ---- pass 2: min-shifted class sums
        for (int qb = 0; qb < nqb; ++qb) {
            const int q = (qb << 6) + lane;
            const bool valid = q < Q;
            cd rr[NRP];
            residual<NRP>(rr, yv, Hw, cons_s, q, NT, NR, lgM, M);
            double rm = INFINITY, rS = 0.0;
            for (int s = 0; s < M; ++s) {
                const double d = dist2<NRP>(rr, hl, cons_s[s]);
                const bool lt = d < rm;
                const double e = fexp_neg(-fabs(d - rm) * inv);
                rS = lt ? fma(rS, e, 1.0) : rS + e;
                rm = lt ? d : rm;
                const double wc = valid ? fexp_neg(-(d - bitsd(cmin[last + s])) * inv) : 0.0;
                const double ws = wave_sum_dpp(wc);
                if (lane == 0) csum[last + s] += ws;
            }
            for (int x = 0; x < NT - 1; ++x) {
                const int sh = lgM * (NT - 2 - x);
                const int dig = (q >> sh) & (M - 1);
                double c = valid ? rS * fexp_neg(-(rm - bitsd(cmin[x * M + dig])) * inv) : 0.0;
                int other = 0;                       // lane bits outside the digit
#pragma unroll
                for (int kb = 0; kb < 6; ++kb)
                    if (kb < sh || kb >= sh + lgM) {
                        c += shfl_xor_d(c, 1 << kb);
                        other |= 1 << kb;
                    }
                if (valid && (lane & other) == 0) csum[x * M + dig] += c;
            }
        }
        wave_sync();

        // ---- outputs
        const size_t sym = bt + t;
        int myidx = 0;
        if (lane < NT) myidx = (bestj >> (lgM * (NT - 1 - lane))) & (M - 1);
        if (lane < NT) {
            if (a.xhat) a.xhat[sym * NT + lane] = cons_s[myidx];
            if (a.idx) a.idx[sym * NT + lane] = myidx;
            if (a.err) {
                const cd xt = a.xd[sym * NT + lane];
                double bd = INFINITY;
                int bi = 0;
                for (int s = 0; s < M; ++s) {
                    const double dx = cabs2(csub(cons_s[s], xt));
                    if (dx < bd) {
                        bd = dx;
                        bi = s;
                    }
                }
                nse += bi != myidx;
                nbe += __popc((unsigned)(lab_s[bi] ^ lab_s[myidx]));
            }
        }
        if (a.post || a.llr) {
            for (int x = 0; x < NT; ++x) {
                const bool in = lane < M;
                const double cm = in ? bitsd(cmin[x * M + lane]) : INFINITY;
                const double cS = in ? csum[x * M + lane] : 0.0;
                if (a.post) {
                    const double ms = wave_min_dpp(cm);
                    const double e = in ? cS * fexp_neg(-(cm - ms) * inv) : 0.0;
                    const double Z = wave_sum_dpp(e);
                    if (in) a.post[(sym * NT + x) * M + lane] = e / Z;
                }
                if (a.llr) {
                    for (int i = 0; i < lgM; ++i) {
                        const bool one = in && ((lab_s[in ? lane : 0] >> i) & 1);
                        const bool zero = in && !one;
                        const double m0 = wave_min_dpp(zero ? cm : INFINITY);
                        const double m1 = wave_min_dpp(one ? cm : INFINITY);
                        double l = (m1 - m0) / s2;
                        if (!a.maxlog) {
                            const double T0 = wave_sum_dpp(zero ? cS * fexp_neg(-(cm - m0) * inv) : 0.0);
                            const double T1 = wave_sum_dpp(one ? cS * fexp_neg(-(cm - m1) * inv) : 0.0);
                            l += log(T0) - log(T1);
                        }
                        if (lane == 0) a.llr[(sym * NT + x) * lgM + i] = l;
                    }
                }
            }
        }
        wave_sync();
    }
    if (a.err && (nse | nbe)) {
        atomicAdd(&a.err[2 * b], nse);
        atomicAdd(&a.err[2 * b + 1], nbe);
    }
}

template <int NRP>
hipError_t launch_nrp(const DetectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(detect_kernel<NRP>, dim3((unsigned)(a.B * a.chunks)), dim3(kHypThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

bool detect_supported(int NT, int NR, int M) {
    return hyp_supported(NT, NR, M) && NT * M <= kMaxCls;
}

hipError_t launch_detect(DetectArgs a, hipStream_t s) {
    a.lgM = hyp_log2(a.M);
    hyp_split(a.NT, a.M, a.Td, a.TC, a.chunks);
    if ((long long)a.B * a.chunks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.err) {
        hipError_t e = hipMemsetAsync(a.err, 0, (size_t)a.B * 2 * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    if (a.NR <= 1) return launch_nrp<1>(a, s);
    if (a.NR <= 2) return launch_nrp<2>(a, s);
    if (a.NR <= 4) return launch_nrp<4>(a, s);
    return launch_nrp<8>(a, s);
}

}  // namespace sbce
