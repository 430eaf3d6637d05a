// The exhaustive enumeration of the J = M^NT hypotheses x_j of a data symbol, shared by the
// detector (detect.hip) and the log-likelihood (loglik.hip): ONE copy of the work split, the
// effective-channel staging and the distance fma sequences, so that both kernels see the same
// distance bits and "trial b of a B-trial call is the B = 1 call" holds for both.
//
// Work split.  One workgroup of 4 waves takes TC consecutive symbols of ONE trial (TC = 4 when
// J >= 4096, else 16; a function of the shape only).  theta of the trial is staged once per
// workgroup in LDS, in tiles of 32 rows of P, and every wave forms the effective channels
// H_t[r][a] = sum_p psi_t[p] theta[(p NT + a) NR + r] of its (up to 4) symbols from each tile.
// Then ONE WAVE PER SYMBOL: with Q = M^(NT-1) prefixes q (streams 0..NT-2) and the last stream s,
// lane l of the wave owns the rows q = 64 qb + l and loops over s; the residual
// y - sum_{a<NT-1} H[:,a] x_a is formed once per row, each distance costs NR complex FMAs.
//
// Not for the E-step units (estep_valu.hip, estep_sweep.hip, estep_sphere.hip, estep_pair.hip,
// estep_pm.hip): they are compiled without NaN honouring and their effective-channel sums have
// their own orders.
#pragma once
#include "sbce_internal.h"

namespace sbce {

constexpr int kHypThreads = 256;
constexpr int kHypWaves = 4;
constexpr int kHypPT = 32;          // rows of P per staged theta tile (even: half = parity of p)
constexpr int kHypMaxSym = 4;       // symbols per wave of a workgroup (TC <= 16)
constexpr int kHypMaxNE = 32;       // NT * NR
constexpr int kHypMaxJ = 65536;

// the shapes the enumeration takes: NT 1..4, NR 1..8 (NT NR <= kHypMaxNE), M^NT <= kHypMaxJ
inline bool hyp_supported(int NT, int NR, int M) {
    if (NT < 1 || NT > 4 || NR < 1 || NR > 8 || M < 2 || M > 64) return false;
    long long J = 1;
    for (int i = 0; i < NT; ++i) J *= M;
    return J <= kHypMaxJ;
}

// log2 of a power of two M (the smallest l with 2^l >= M otherwise)
inline int hyp_log2(int M) {
    int l = 0;
    while ((1 << l) < M) ++l;
    return l;
}

// symbols per workgroup and workgroups per trial
inline void hyp_split(int NT, int M, int Td, int& TC, int& chunks) {
    long long J = 1;
    for (int i = 0; i < NT; ++i) J *= M;
    TC = J >= 4096 ? kHypWaves : kHypWaves * kHypMaxSym;
    chunks = (Td + TC - 1) / TC;
}

__device__ __forceinline__ cd shfl_xor_c(cd v, int m) {
    return cmk(shfl_xor_d(v.x, m), shfl_xor_d(v.y, m));
}

// ||r - h c||^2 over the NRP (padded, zero) rows, in one fixed fma sequence: every pass of every
// kernel gets the same bits
template <int NRP>
__device__ __forceinline__ double dist2(const cd* r, const cd* h, cd c) {
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < NRP; ++i) {
        double tx = fma(-h[i].x, c.x, r[i].x);
        tx = fma(h[i].y, c.y, tx);
        double ty = fma(-h[i].x, c.y, r[i].y);
        ty = fma(-h[i].y, c.x, ty);
        d = fma(tx, tx, d);
        d = fma(ty, ty, d);
    }
    return d;
}

// the row's residual y - sum_{a < NT-1} H[:,a] cons[digit_a(q)]
template <int NRP>
__device__ __forceinline__ void residual(cd* rr, const cd* yv, const cd* Hw, const cd* cons_s,
                                         int q, int NT, int NR, int lgM, int M) {
#pragma unroll
    for (int i = 0; i < NRP; ++i) rr[i] = yv[i];
    for (int a = 0; a < NT - 1; ++a) {
        const cd c = cons_s[(q >> (lgM * (NT - 2 - a))) & (M - 1)];
#pragma unroll
        for (int i = 0; i < NRP; ++i) {
            const cd h = csel(i < NR, Hw[a * NR + (i < NR ? i : 0)], czero());
            rr[i].x = fma(-h.x, c.x, rr[i].x);
            rr[i].x = fma(h.y, c.y, rr[i].x);
            rr[i].y = fma(-h.x, c.y, rr[i].y);
            rr[i].y = fma(-h.y, c.x, rr[i].y);
        }
    }
}

// Effective channels of the symbols t0 + w + 4 k < tend of trial b into H_s[w][k][], theta staged
// tile by tile through th_s (kHypPT * kHypMaxNE values).  Every thread of the workgroup calls it
// with its tid, lane = tid & 63 and w = tid >> 6; the caller's barrier follows.  lane = (entry,
// half): the half-sums run over even / odd p in ascending order and are added even + odd.
__device__ __forceinline__ void heff_stage(cd (&H_s)[kHypWaves][kHypMaxSym][kHypMaxNE],
                                           cd (&th_s)[kHypPT * kHypMaxNE], const cd* theta,
                                           const cd* psid, int b, size_t bt, int P, int NE, int t0,
                                           int tend, int tid, int lane, int w) {
    const cd* th = theta + (size_t)b * P * NE;
    const int e = lane & 31, half = lane >> 5;
    cd acc[kHypMaxSym];
#pragma unroll
    for (int k = 0; k < kHypMaxSym; ++k) acc[k] = czero();
    for (int p0 = 0; p0 < P; p0 += kHypPT) {
        const int np = P - p0 < kHypPT ? P - p0 : kHypPT;
        __syncthreads();
        for (int i = tid; i < np * NE; i += kHypThreads) th_s[i] = th[(size_t)p0 * NE + i];
        __syncthreads();
        if (e < NE) {
#pragma unroll
            for (int k = 0; k < kHypMaxSym; ++k) {
                const int t = t0 + w + kHypWaves * k;
                if (t < tend) {
                    const cd* ps = psid + (bt + t) * P + p0;
                    for (int pp = half; pp < np; pp += 2)
                        acc[k] = cfma(acc[k], ps[pp], th_s[pp * NE + e]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kHypMaxSym; ++k) {
        const cd o = shfl_xor_c(acc[k], 32);
        if (half == 0 && e < NE) H_s[w][k][e] = cadd(acc[k], o);   // even + odd
    }
}

}  // namespace sbce
