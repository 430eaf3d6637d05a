// Device code shared by the linear kernel family -- the soft ZF / MMSE, EP and soft-input EP
// E-steps (estep_linear.hip) and the linear soft detector (detect_linear.hip): the work split of a
// workgroup over its 32 symbols, the table in LDS, the staging of H_t, the per-symbol Cholesky with
// its folded forward substitution, the per-stream estimate, the plain soft demapper and the
// product-form moment store; and the host-side dispatch on n_tx.  The work split is described in
// detect_linear.hip's header comment; every kernel runs these steps operation for operation, so
// x_soft and nu of the ZF / MMSE detector and E-step are the same bits.
#pragma once

#include <type_traits>

#include "sbce_internal.h"

namespace sbce {

constexpr int kLinThreads = 256;
constexpr int kLinSym = 32;         // symbols per workgroup: 4 waves x 8 lane groups
constexpr int kLinPT = 32;          // rows of P per staged tile
constexpr int kLinMaxNE = 64;       // NT * NR
constexpr int kLinHS = 65;          // row stride of H_s (one 16-byte slot of padding)
constexpr int kLinBuf = kLinPT * kLinMaxNE + kLinSym * kLinPT;   // theta tile + psi tile >= 32 * 65

__device__ __forceinline__ cd bperm_c(cd v, int addr) {
    return cmk(bperm_d(v.x, addr), bperm_d(v.y, addr));
}
// max over each group of 8 lanes (quad xor 1, xor 2, then the mirrored quad)
__device__ __forceinline__ double group8_max(double v) {
    v = fmax(v, dpp_d<0xB1>(v));
    v = fmax(v, dpp_d<0x4E>(v));
    return fmax(v, dpp_d<0x141>(v));
}

// The work of one lane: workgroup blockIdx.x takes the symbols t0 .. tend - 1 of trial b (chunk
// blockIdx.x % chunks), a group of 8 lanes per symbol, lane aa = column aa of the symbol's matrix.
// Lanes past NT and groups past the chunk repeat a valid column and a valid symbol (no divergence
// around the cross-lane moves, no read outside the trial) and store nothing: act is false.
struct LinSplit {
    int b, t0, tend;
    size_t bt;         // b * Td: the trial's first symbol
    int lane, aa, k;   // lane of the wave, column, row of H_s
    bool act;
    size_t sym;        // bt + t0 + k
};
__device__ __forceinline__ LinSplit lin_split(int NT, int Td, int chunks) {
    LinSplit sp;
    sp.b = blockIdx.x / chunks;
    sp.t0 = (blockIdx.x % chunks) * kLinSym;
    sp.tend = sp.t0 + kLinSym < Td ? sp.t0 + kLinSym : Td;
    sp.bt = (size_t)sp.b * Td;
    const int tid = threadIdx.x, w = tid >> 6;
    sp.lane = tid & 63;
    const int grp = sp.lane >> 3, al = sp.lane & 7;
    const int ts = sp.t0 + w * 8 + grp;
    sp.act = al < NT && ts < sp.tend;
    sp.aa = al < NT ? al : 0;
    sp.k = ts < sp.tend ? w * 8 + grp : sp.tend - 1 - sp.t0;
    sp.sym = sp.bt + sp.t0 + sp.k;
    return sp;
}

// The table, and the labels where the kernel keeps them (lab_s null: it does not; labels null: the
// identity), to LDS.  lin_stage_h's barriers publish them.
__device__ __forceinline__ void lin_load_table(cd* cons_s, int* lab_s, const cd* cons,
                                               const int32_t* labels, int M) {
    const int tid = threadIdx.x;
    if (tid < M) {
        cons_s[tid] = cons[tid];
        if (lab_s) lab_s[tid] = labels ? labels[tid] : tid;
    }
}

// es = mean |cons|^2 from the table in LDS: one ascending-s sum, the same bits on every lane
__device__ __forceinline__ double lin_table_energy(const cd* cons_s, int M) {
    double es = 0.0;
    for (int s = 0; s < M; ++s) es += cabs2(cons_s[s]);
    return es / (double)M;
}

// Staging: H_t of the symbols t0 .. tend - 1 of one trial into buf_s[kLinBuf], row k = symbol
// t0 + k at stride kLinHS, entry e = a * NR + r.  th: the trial's theta; psi: the trial's phases
// [Td][P].  Every thread of the 256-thread block calls it; it starts and ends with a barrier.
__device__ __forceinline__ void lin_stage_h(cd* buf_s, const cd* th, const cd* psi, int NE, int P,
                                            int t0, int tend) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    cd* th_s = buf_s;
    cd* psi_s = buf_s + kLinPT * kLinMaxNE;
    int lgE = 0;
    while ((1 << lgE) < NE) ++lgE;
    const int ng = (64 >> lgE) < 8 ? (64 >> lgE) : 8;   // symbol subsets per wave
    const int nj = 8 / ng;                              // symbols per lane
    const int e = lane & ((1 << lgE) - 1), g = lane >> lgE;
    const bool on = e < NE && g < ng;
    cd acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = czero();
    for (int p0 = 0; p0 < P; p0 += kLinPT) {
        const int np = P - p0 < kLinPT ? P - p0 : kLinPT;
        __syncthreads();
        for (int i = tid; i < np * NE; i += kLinThreads) th_s[i] = th[(size_t)p0 * NE + i];
        for (int i = tid; i < kLinSym * kLinPT; i += kLinThreads) {
            const int k = i >> 5, pp = i & 31;
            psi_s[i] = (t0 + k < tend && pp < np) ? psi[(size_t)(t0 + k) * P + p0 + pp] : czero();
        }
        __syncthreads();
        if (on) {
            const cd* ps = psi_s + (w * 8 + g) * kLinPT;
            for (int pp = 0; pp < np; ++pp) {
                const cd tv = th_s[pp * NE + e];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < nj) acc[j] = cfma(acc[j], ps[j * ng * kLinPT + pp], tv);
            }
        }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nj) buf_s[(w * 8 + g + j * ng) * kLinHS + e] = acc[j];
    }
    __syncthreads();
}

// Solve of one symbol by its group of 8 lanes, lane column aa (lanes past NT repeat column 0: no
// divergence around the cross-lane moves).  Hs: the symbol's row of H_s; y: its observation [NR].
// Out: g = (A^-1)_aa, z = (A^-1 H^H y)_aa, fail = a pivot <= 1e-14 max_a A_aa (the whole group
// agrees on it).
template <int NT>
__device__ __forceinline__ void lin_solve(const cd* Hs, const cd* y, int NR, int aa, int lane,
                                          double rho, double& g, cd& z, bool& fail) {
    cd c[NT + 1];
#pragma unroll
    for (int i = 0; i <= NT; ++i) c[i] = czero();
    for (int r = 0; r < NR; ++r) {
        const cd ha = Hs[aa * NR + r];
#pragma unroll
        for (int i = 0; i < NT; ++i) c[i] = cfmac(c[i], ha, Hs[i * NR + r]);   // conj(H[r][i]) H[r][a]
        c[NT] = cfmac(c[NT], ha, y[r]);                                        // conj((H^H y)_a)
    }
    double diag = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const bool d = i == aa;
        c[i].x = d ? c[i].x + rho : c[i].x;
        diag = d ? c[i].x : diag;
    }
    const double tol = 1e-14 * group8_max(diag);

    cd wv[NT];                       // forward substitution L w = e_a, in place
#pragma unroll
    for (int i = 0; i < NT; ++i) wv[i] = cmk(i == aa ? 1.0 : 0.0, 0.0);
    fail = false;
    g = 0.0;
    z = czero();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int addr = ((lane & 56) | j) << 2;
        const double piv = bperm_d(c[j].x, addr);
        fail = fail || !(piv > tol);
        const double rinv = fast_rsqrt64(piv);
        cd lj[NT + 1];
        cd laj = czero();
#pragma unroll
        for (int i = j + 1; i <= NT; ++i) {
            lj[i] = cscale(bperm_c(c[i], addr), rinv);
            if (i < NT) laj = csel(i == aa, lj[i], laj);
        }
        const cd wj = cscale(wv[j], rinv);
        g = fma(wj.x, wj.x, g);
        g = fma(wj.y, wj.y, g);
        z = cfmac(z, cconj(wj), lj[NT]);                // conj(w_j) u_j, u_j = conj(lj[NT])
#pragma unroll
        for (int i = j + 1; i <= NT; ++i) {
            c[i] = cfmac(c[i], cmk(-lj[i].x, -lj[i].y), laj);
            if (i < NT) wv[i] = cfma(wv[i], cmk(-lj[i].x, -lj[i].y), wj);
        }
    }
}

// The stream's unbiased estimate xs, its effective noise variance nu and inv = 1 / nu.  A failed
// symbol, or an MMSE stream the channel does not carry (mu <= 0), gets xs = 0, nu = +inf, inv = 0:
// every demapper weight is then 1 (the uniform posterior).
__device__ __forceinline__ void lin_estimate(bool mmse, double rho, double s2, double g, cd z,
                                             bool fail, cd& xs, double& nu, double& inv) {
    xs = z;
    nu = s2 * g;
    bool dead = false;
    if (mmse) {
        const double mu = fma(-rho, g, 1.0);
        const double rmu = 1.0 / mu;
        xs = cscale(z, rmu);
        nu *= rmu;
        dead = !(mu > 0.0);                             // a stream the channel does not carry
    }
    dead = dead || fail;                                // fail alone flags the trial
    if (dead) {
        xs = czero();
        nu = INFINITY;
    }
    inv = dead ? 0.0 : 1.0 / nu;
}

// The soft demapper of stream a on (xs, inv = 1 / nu): one scan of the table for the minimum
// distance, one for the min-shifted sums (the nearest point has weight 1: nothing is 0 / 0).  Out:
// the posterior mean and second moment.
__device__ __forceinline__ void lin_demap(const cd* cons_s, int M, cd xs, double inv, cd& mean,
                                          double& saa) {
    double dmin = INFINITY;
    for (int s = 0; s < M; ++s) dmin = fmin(dmin, cabs2(csub(xs, cons_s[s])));
    double Z = 0.0;
    saa = 0.0;
    mean = czero();
    for (int s = 0; s < M; ++s) {
        const cd cs = cons_s[s];
        const double e = fexp_neg(-(cabs2(csub(xs, cs)) - dmin) * inv);
        Z += e;
        mean = caxpy(mean, e, cs);
        saa = fma(e, cabs2(cs), saa);
    }
    mean = cmk(mean.x / Z, mean.y / Z);
    saa /= Z;
}

// The symbol's moments in the product form, mom [B][Td][NT + NT*NT]: m_a = mean, S[a][a] = saa,
// S[a][q] = m_a conj(m_q).  Every lane of the wave calls it (the cross-lane moves see every lane);
// the active ones store.
template <int NT>
__device__ __forceinline__ void lin_store_moments(cd* mom, const LinSplit& sp, cd mean,
                                                  double saa) {
    cd* mo = mom + sp.sym * (NT + NT * NT);
    if (sp.act) mo[sp.aa] = mean;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const cd mq = bperm_c(mean, ((sp.lane & 56) | q) << 2);
        if (sp.act) mo[NT + sp.aa * NT + q] = q == sp.aa ? cmk(saa, 0.0) : cmulc(mean, mq);
    }
}

// f(std::integral_constant<int, NT>{}) for NT = 1 .. 8: the launchers' dispatch on n_tx
template <class F>
hipError_t lin_dispatch_nt(int NT, F f) {
    switch (NT) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return hipErrorInvalidValue;
}

}  // namespace sbce
