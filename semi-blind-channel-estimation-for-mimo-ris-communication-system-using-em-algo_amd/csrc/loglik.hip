// Observed-data log-likelihood (sbce_loglik) and the truth-free convergence stop of the EM chain
// (sbce_em_conv), DESIGN.md §3.10.  Per trial b with s2 = varn_b^2 and J = M^NT hypotheses x_j
// (itertools.product order, first stream slowest), d_j = ||y_t - H_t x_j||^2 with the effective
// channel H_t[r][a] = sum_p psi_t[p] theta[(p NT + a) NR + r]:
//   ll_sym[b][t] = -d_min/s2 + log sum_j e^{-(d_j - d_min)/s2} - log J - NR log(pi s2)
//   ll[b]        = sum_t ll_sym[b][t] + sum_pilots ( -||y_p - H_c u_p||^2/s2 - NR log(pi s2) )
//
// loglik_sym_kernel   grid B chunks + B npb workgroups of 4 waves.
//   Symbol workgroups (the first B chunks) use the work split, the effective channels and the
//   distance arithmetic of hyp_enum.h (shared with detect.hip): TC consecutive symbols of ONE
//   trial, then ONE WAVE PER SYMBOL: lane l owns the prefix rows q = 64 qb + l (streams 0..NT-2)
//   and loops over the last stream.
//   Only one scalar per symbol is wanted, so a lane keeps ONE online log-sum-exp pair (rm, rS)
//   over all its hypotheses (rS = sum e^{-(d - rm)/s2}, rescaled when rm drops) and the wave
//   combines the 64 pairs once: m = wave min of rm, S = DPP wave sum of rS e^{-(rm - m)/s2}.
//   There are no class minima, no LDS atomics and no second distance pass.  The lane that holds
//   the minimum contributes a term equal to 1, so S >= 1 and every output is finite.
//   A term with (d - rm)/s2 >= 50 for EVERY lane of the wave is skipped (rm >= d_min, so the
//   dropped term is below e^-50 of the sum: over J <= 65536 terms less than 2e-17 relative).
//   Pilot workgroups (the last B npb): item i = 256 k + tid is (pilot t, antenna r), r fastest,
//   as noise.hip's pilot items (the same p-then-a fma order, there on tiles of 8 phases); theta
//   walks the same LDS tiles, u_p is read from global memory.  The block sum of
//   ||y_p - H_c u_p||^2 (DPP wave sums, then the four waves in order: block_sum4) goes to
//   ppart[b][k].
// loglik_final_kernel one wave per trial: lane l adds ll_sym[b][l], [l + 64], ... in ascending
//   order, one DPP wave sum, then lane 0 adds the pilot block sums in index order.
// Determinism: no floating-point atomic; every order above is fixed by the shape alone and
//   nothing is shared between trials, so trial b of a B-trial call is bitwise the B = 1 call.
//
// conv_step_kernel    one workgroup per trial, after an iteration's M-step (and noise update and
//   log-likelihood): ||theta - theta_prev||^2 and ||theta||^2 (thread-strided partial sums in
//   ascending order, DPP wave sums, the four waves in order), the histories, theta_prev = theta
//   and the stop decision in product form (no division; a NaN compares false and never stops).
#include "hyp_enum.h"

namespace sbce {

namespace {

constexpr double kSkip = 50.0;      // (d - rm)/s2 at which a term is dropped

template <int NRP>
__global__ __launch_bounds__(kHypThreads) void loglik_sym_kernel(LoglikArgs a) {
    __shared__ cd th_s[kHypPT * kHypMaxNE];
    __shared__ cd cons_s[64];
    __shared__ cd H_s[kHypWaves][kHypMaxSym][kHypMaxNE];
    __shared__ double red[kHypWaves];

    const int NT = a.NT, NR = a.NR, P = a.P, Td = a.Td, M = a.M, lgM = a.lgM;
    const int NE = NT * NR;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nsym = a.B * a.chunks;

    if ((int)blockIdx.x >= nsym) {
        // ---- pilot residuals: 256 (pilot, antenna) items of one trial
        const int pi = (int)blockIdx.x - nsym;
        const int b = pi / a.npb, k = pi - b * a.npb;
        if (a.done && a.done[b]) return;                 // block-uniform: the trial has stopped
        const int Tp = a.Tp;
        const int i = k * kHypThreads + tid;
        const bool act = i < Tp * NR;
        const int t = act ? i / NR : 0, r = act ? i - t * NR : 0;
        const cd* th = a.theta + (size_t)b * P * NE;
        const cd* upg = a.up + ((size_t)b * Tp + t) * ((size_t)P * NT);
        cd h = czero();                                  // (H_c u_p)_r
        for (int p0 = 0; p0 < P; p0 += kHypPT) {
            const int np = P - p0 < kHypPT ? P - p0 : kHypPT;
            __syncthreads();
            for (int e = tid; e < np * NE; e += kHypThreads) th_s[e] = th[(size_t)p0 * NE + e];
            __syncthreads();
            if (act)
                for (int pp = 0; pp < np; ++pp)
                    for (int ai = 0; ai < NT; ++ai)
                        h = cfma(h, th_s[(pp * NT + ai) * NR + r], upg[(p0 + pp) * NT + ai]);
        }
        double q = act ? cabs2(csub(a.yp[((size_t)b * Tp + t) * NR + r], h)) : 0.0;
        q = block_sum4(wave_sum_dpp(q), red, lane, w);
        if (tid == 0) a.ppart[(size_t)b * a.npb + k] = q;
        return;
    }

    const int b = blockIdx.x / a.chunks, ch = blockIdx.x % a.chunks;
    if (a.done && a.done[b]) return;                     // block-uniform
    const int t0 = ch * a.TC;
    const int tend = t0 + a.TC < Td ? t0 + a.TC : Td;
    const size_t bt = (size_t)b * Td;

    if (tid < M) cons_s[tid] = a.cons[tid];

    heff_stage(H_s, th_s, a.theta, a.psid, b, bt, P, NE, t0, tend, tid, lane, w);
    __syncthreads();

    const int Q = 1 << (lgM * (NT - 1));
    const int nqb = (Q + 63) >> 6;
    const double v = a.varn_t ? a.varn_t[b] : a.varn;
    const double s2 = v * v;
    const double inv = 1.0 / s2;
    const double thr = kSkip * s2;
    const double cst = log((double)Q * (double)M) + (double)NR * log(M_PI * s2);
    // Q is a power of two: below 64 there is one row block and the lanes past Q own nothing,
    // from 64 on every lane owns a row of every block
    const bool valid = lane < Q;

    for (int k = 0; k < kHypMaxSym; ++k) {
        const int t = t0 + w + kHypWaves * k;
        if (t >= tend) break;                            // wave-uniform
        const cd* Hw = H_s[w][k];
        cd yv[NRP], hl[NRP];
#pragma unroll
        for (int i = 0; i < NRP; ++i) {
            const int ic = i < NR ? i : 0;
            yv[i] = csel(i < NR, a.yd[(bt + t) * NR + ic], czero());
            hl[i] = csel(i < NR, Hw[(NT - 1) * NR + ic], czero());
        }
        double rm = INFINITY, rS = 0.0;                  // the lane's online log-sum-exp pair
        for (int qb = 0; qb < nqb; ++qb) {
            const int q = (qb << 6) + lane;
            cd rr[NRP];
            residual<NRP>(rr, yv, Hw, cons_s, q, NT, NR, lgM, M);
            for (int s = 0; s < M; ++s) {
                const double d = dist2<NRP>(rr, hl, cons_s[s]);
                if (!__any(d - rm < thr)) continue;      // below e^-50 of every lane's sum
                const bool lt = d < rm;
                const double e = fexp_neg(-fabs(d - rm) * inv);
                rS = lt ? fma(rS, e, 1.0) : rS + e;
                rm = lt ? d : rm;
            }
        }
        if (!valid) {
            rm = INFINITY;
            rS = 0.0;
        }
        const double m = wave_min_dpp(rm);
        const double S = wave_sum_dpp(rS * fexp_neg(-(rm - m) * inv));
        if (lane == 0) a.sym[bt + t] = (log(S) - m * inv) - cst;
    }
}

__global__ __launch_bounds__(kHypThreads) void loglik_final_kernel(LoglikArgs a) {
    const int b = blockIdx.x * kHypWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= a.B) return;                                // wave-uniform
    if (a.done && a.done[b]) return;
    double acc = 0.0;
    for (int t = lane; t < a.Td; t += 64) acc += a.sym[(size_t)b * a.Td + t];
    acc = wave_sum_dpp(acc);
    if (lane == 0) {
        double qp = 0.0;
        for (int k = 0; k < a.npb; ++k) qp += a.ppart[(size_t)b * a.npb + k];
        const double v = a.varn_t ? a.varn_t[b] : a.varn;
        const double s2 = v * v;
        a.ll[b] = acc + (-qp / s2 - (double)a.Tp * (double)a.NR * log(M_PI * s2));
    }
}

template <int NRP>
hipError_t launch_sym(const LoglikArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(loglik_sym_kernel<NRP>, dim3((unsigned)(a.B * (a.chunks + a.npb))),
                       dim3(kHypThreads), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void conv_init_kernel(const cd* theta, cd* prev, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) prev[i] = theta[i];
}

__global__ __launch_bounds__(256) void conv_step_kernel(ConvArgs c) {
    __shared__ double sh[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t hi = (size_t)b * c.iters + c.it;
    if (c.done[b]) {                                     // stopped: the histories keep their value
        if (tid == 0) {                                  // (a stop needs it >= 1: min_iters >= 1)
            if (c.dth_hist) c.dth_hist[hi] = c.dth_hist[hi - 1];
            if (c.ll_hist) c.ll_hist[hi] = c.ll_hist[hi - 1];
        }
        return;
    }
    const cd* th = c.theta + (size_t)b * c.K;
    cd* pv = c.prev + (size_t)b * c.K;
    double nd = 0.0, nt = 0.0;
    for (int e = tid; e < c.K; e += 256) {
        const cd x = th[e];
        nd += cabs2(csub(x, pv[e]));
        nt += cabs2(x);
        pv[e] = x;
    }
    nd = wave_sum_dpp(nd);
    nt = wave_sum_dpp(nt);
    if ((tid & 63) == 0) {
        sh[tid >> 6] = nd;
        sh[4 + (tid >> 6)] = nt;
    }
    __syncthreads();
    if (tid == 0) {
        nd = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        nt = ((sh[4] + sh[5]) + sh[6]) + sh[7];
        if (c.dth_hist) c.dth_hist[hi] = sqrt(nd / nt);
        bool stop = nd <= c.tol_theta2 * nt;
        if (c.ll_hist) {
            const double ll = c.ll_cur[b];
            c.ll_hist[hi] = ll;
            if (c.tol_ll > 0.0 && c.it >= 1 && ll - c.ll_hist[hi - 1] <= c.tol_ll * fabs(ll))
                stop = true;
        }
        if (c.iters_done) c.iters_done[b] = c.it + 1;
        if (stop && c.it + 1 >= c.min_iters) {
            c.done[b] = 1;
            if (c.status) c.status[b] |= SBCE_STATUS_CONVERGED;
        }
    }
}

}  // namespace

bool loglik_supported(const Problem& pb) {
    if (pb.M > 64 || (pb.M & (pb.M - 1))) return false;  // the table is indexed by bit fields
    return hyp_supported(pb.NT, pb.NR, pb.M);
}

int loglik_npb(const Problem& pb) {
    return (int)(((long)pb.Tp * pb.NR + kHypThreads - 1) / kHypThreads);
}

hipError_t launch_loglik(const Problem& pb, LoglikArgs a, hipStream_t s) {
    a.B = pb.B; a.NT = pb.NT; a.NR = pb.NR; a.P = pb.P; a.Tp = pb.Tp; a.Td = pb.Td; a.M = pb.M;
    a.varn = pb.varn;
    a.lgM = hyp_log2(pb.M);
    hyp_split(pb.NT, pb.M, pb.Td, a.TC, a.chunks);
    a.npb = loglik_npb(pb);
    if ((long long)pb.B * (a.chunks + a.npb) > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e;
    if (pb.NR <= 1) e = launch_sym<1>(a, s);
    else if (pb.NR <= 2) e = launch_sym<2>(a, s);
    else if (pb.NR <= 4) e = launch_sym<4>(a, s);
    else e = launch_sym<8>(a, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(loglik_final_kernel, dim3((pb.B + kHypWaves - 1) / kHypWaves),
                       dim3(kHypThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv_init(const Problem& pb, const cd* theta, cd* prev, hipStream_t s) {
    const size_t n = (size_t)pb.B * pb.K;
    hipLaunchKernelGGL(conv_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, theta,
                       prev, n);
    return hipGetLastError();
}

hipError_t launch_conv_step(const Problem& pb, ConvArgs c, hipStream_t s) {
    c.K = pb.K;
    hipLaunchKernelGGL(conv_step_kernel, dim3(pb.B), dim3(256), 0, s, c);
    return hipGetLastError();
}

}  // namespace sbce
