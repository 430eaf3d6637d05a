// The one-thread-per-symbol passes in front of the MFMA sweep (estep_sweep.hip): the preparation
// pass, or the sphere pass (search tree, enumeration, tile bounds of the symbols it lists).
#include "sbce_internal.h"

namespace sbce {

namespace {

// ============================================================================
// Per-symbol preparation pass (one THREAD per symbol) for the MFMA sweep: H_eff(t), the
// candidate bound of candidate_distance and the column-tile bounds of column_tile_bounds
// (both estep_sweep.hip), written to the workspace (PrepLayout).  These are short dependent chains (a 4 x 4
// Cholesky, a Gram-Schmidt, M-way minima): inside the sweep kernel one wave would run
// them serially per symbol; here 64 symbols run them side by side per wave.
// ============================================================================
struct PrepConst {
    int B, Td, P, M, lm, nkt, stride;
    int uni;           // wave-uniform theta loads (SBCE_PREP_UNI=0 disables: A/B runs)
    double reg;
    // sphere pass (estep_sphere_kernel; EstepArgs::list receives the symbols it leaves)
    int budget;        // DFS steps per symbol before the symbol is left to the sweep
    int count;         // SBCE_ESTEP_COUNT=1: tally resolved / listed symbols (g_estep_sphere)
    int hard;          // hard (argmin) E-step: sphere radius without the soft threshold
    int pair;          // route wide-tree symbols that pass the screen to the factorised pass
    double inv_s2, thr_d;
};

// Diagnostic (SBCE_ESTEP_COUNT=1): symbols the sphere pass's enumeration resolved, symbols it
// left to the MFMA sweep, and symbols the tree pass resolved alone (single surviving path).
__device__ unsigned long long g_estep_sphere[3];

// ---- H_eff(t) = sum_p psi_p H_p (theta of the symbol's trial, psi of the symbol) ----
template <int NT, int NR>
__device__ __forceinline__ void heff_load(const EstepArgs& a, const PrepConst& c, long gsym, int b,
                                          cd (&H)[NT][NR]) {
    constexpr int NO = NT * NR;
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < NR; ++r) H[q][r] = czero();
    const cd* ps = a.psid + (size_t)gsym * c.P;
    // the wave's 64 symbols normally belong to one trial: theta's address is then
    // wave-uniform and its loads go through the scalar cache (one vector load per p)
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    if (c.uni && __all(b == b0)) {
        const cd* th = a.theta + (size_t)b0 * c.P * NO;
#pragma unroll 8
        for (int p = 0; p < c.P; ++p) {
            const cd psi = ps[p];
#pragma unroll
            for (int q = 0; q < NT; ++q)
#pragma unroll
                for (int r = 0; r < NR; ++r) H[q][r] = cfma(H[q][r], psi, th[p * NO + q * NR + r]);
        }
    } else {
        const cd* th = a.theta + (size_t)b * c.P * NO;
        for (int p = 0; p < c.P; ++p) {
            const cd psi = ps[p];
#pragma unroll
            for (int q = 0; q < NT; ++q)
#pragma unroll
                for (int r = 0; r < NR; ++r) H[q][r] = cfma(H[q][r], psi, th[p * NO + q * NR + r]);
        }
    }
}

// Ridge Cholesky G + reg I = L L^H of G = H^H H (L strictly lower in Lm, pivots piv,
// 1/sqrt(pivots) dinv) and zf = L^-1 H^H y.
template <int NT, int NR>
__device__ __forceinline__ void ridge_chol(const cd (&H)[NT][NR], const cd (&y)[NR], double reg,
                                           cd (&Lm)[NT][NT], double (&piv)[NT], double (&dinv)[NT],
                                           cd (&zf)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        cd gjj = czero();
#pragma unroll
        for (int r = 0; r < NR; ++r) gjj = cfmac(gjj, H[j][r], H[j][r]);
        double d = gjj.x + reg;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= cabs2(Lm[j][k]);
        piv[j] = fmax(d, 1e-300);
        const double inv = fast_rsqrt(piv[j]);
        dinv[j] = inv;
#pragma unroll
        for (int i = j + 1; i < NT; ++i) {
            cd s = czero();
#pragma unroll
            for (int r = 0; r < NR; ++r) s = cfmac(s, H[j][r], H[i][r]);   // G[i][j]
#pragma unroll
            for (int k = 0; k < j; ++k) s = csub(s, cmulc(Lm[i][k], Lm[j][k]));
            Lm[i][j] = cscale(s, inv);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        cd s = czero();
#pragma unroll
        for (int r = 0; r < NR; ++r) s = cfmac(s, y[r], H[i][r]);          // (H^H y)_i
#pragma unroll
        for (int k = 0; k < i; ++k) s = csub(s, cmul(Lm[i][k], zf[k]));
        zf[i] = cscale(s, dinv[i]);
    }
}

// Candidate of candidate_distance (same arithmetic order): quantised ridge LS estimate from
// the factorisation above; returns its distance d0 and the magnitude scale sc.
template <int NT, int NR>
__device__ __forceinline__ double prep_candidate(const cd (&H)[NT][NR], const cd (&y)[NR],
                                                 const cd (&Lm)[NT][NT], const double (&dinv)[NT],
                                                 const cd (&zf)[NT], const cd* cons, int M,
                                                 double& sc, int& xidx) {
    cd x[NT];
    xidx = 0;
    cd z[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) z[i] = zf[i];
#pragma unroll
    for (int i = NT - 1; i >= 0; --i) {
        cd s = z[i];
#pragma unroll
        for (int k = i + 1; k < NT; ++k) s = csub(s, cmul(cconj(Lm[k][i]), z[k]));
        z[i] = cscale(s, dinv[i]);
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        double bd = INFINITY;
        int bs = 0;
        #pragma unroll 4
        for (int s = 0; s < M; ++s) {
            const double dd = cabs2(csub(z[q], cons[s]));
            if (dd < bd) { bd = dd; bs = s; }
        }
        x[q] = cons[bs];
        xidx |= bs << (8 * q);
    }
    double d0 = 0.0;
    sc = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        cd res = y[r];
        sc += cabs2(res);
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const cd hx = cmul(H[q][r], x[q]);
            res = csub(res, hx);
            sc += NT * cabs2(hx);
        }
        d0 += cabs2(res);
    }
    return d0;
}

// Screen of the factorised-weight pass (estep_pair.hip), NT = 4: an UPPER bound of its range
// D = sum_f (max f - f(x_c)) over the six log tables, from the candidate x_c alone:
//   max A <= 0                        ->  A term <= ||y - h_0 x_c0 - h_1 x_c1||^2 / s2,
//   max B <= ||y||^2 / s2             ->  B term <= ||y - h_2 x_c2 - h_3 x_c3||^2 / s2,
//   max E_ab <= 2 |h_a^H h_b| max|c|^2 / s2.
// The enumeration routes a symbol it gives up on to the pass only when this bound is within the
// pass's limit, so the pass never has to hand a symbol back.
// Returns the x_c-dependent part (in units of 1/s2) and sets gsum >= sum_ab 2 |h_a^H h_b|, the
// coefficient of max|c|^2 (known after the Babai descent): D <= (part + gsum max|c|^2) / s2.
template <int NT, int NR>
__device__ __forceinline__ double pair_screen(const cd (&H)[NT][NR], const cd (&y)[NR], int xidx,
                                              const cd* cons, double& gsum) {
    gsum = 0.0;
    if constexpr (NT != 4) {
        return INFINITY;
    } else {
        cd x[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) x[q] = cons[(xidx >> (8 * q)) & 255];
        double na = 0.0, nb = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            na += cabs2(csub(csub(y[r], cmul(H[0][r], x[0])), cmul(H[1][r], x[1])));
            nb += cabs2(csub(csub(y[r], cmul(H[2][r], x[2])), cmul(H[3][r], x[3])));
        }
        double up = na + nb;
#pragma unroll
        for (int a0 = 0; a0 < 2; ++a0)
#pragma unroll
            for (int b0 = 2; b0 < 4; ++b0) {
                cd G = czero();
#pragma unroll
                for (int r = 0; r < NR; ++r) G = cfmac(G, H[b0][r], H[a0][r]);    // h_a^H h_b
                const cd t = cmul(G, x[b0]);
                gsum += 2.0 * (fabs(G.x) + fabs(G.y));                      // >= 2 |G|
                up += 2.0 * fma(x[a0].x, t.x, x[a0].y * t.y);               // -E_ab(x_c) s2
            }
        return up;
    }
}

// NT = 2, square QAM (estep_pair.hip estep_fact2_kernel): D = (sum of the eight log-table maxima)
// - l(x_c), both times 1/s2, with x_c the prep candidate (a real hypothesis: l(x_c) <= max l).  The
// 1-D tables' maxima over the constellation's real / imaginary parts, the bilinear ones at the
// corners of the level box.  The factorised pass represents every weight within e^-50 of the
// largest as a normal double when D <= kPairDmax.
template <int NR>
__device__ __forceinline__ double fact2_bound(const cd (&H)[2][NR], const cd (&y)[NR], int xidx,
                                              const cd* cons, int M, double inv_s2) {
    cd z0 = czero(), z1 = czero(), g = czero();
    double g00 = 0.0, g11 = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        z0 = cfmac(z0, y[r], H[0][r]);
        z1 = cfmac(z1, y[r], H[1][r]);
        g = cfmac(g, H[1][r], H[0][r]);
        g00 += cabs2(H[0][r]);
        g11 += cabs2(H[1][r]);
    }
    double fa0 = -INFINITY, fb0 = -INFINITY, fa1 = -INFINITY, fb1 = -INFINITY;
    double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
    for (int s = 0; s < M; ++s) {
        const double av = cons[s].x, bv = cons[s].y;
        fa0 = fmax(fa0, 2.0 * av * z0.x - g00 * av * av);
        fb0 = fmax(fb0, 2.0 * bv * z0.y - g00 * bv * bv);
        fa1 = fmax(fa1, 2.0 * av * z1.x - g11 * av * av);
        fb1 = fmax(fb1, 2.0 * bv * z1.y - g11 * bv * bv);
        amin = fmin(amin, av); amax = fmax(amax, av);
        bmin = fmin(bmin, bv); bmax = fmax(bmax, bv);
    }
    auto corner = [](double k, double u0, double u1, double v0, double v1) {
        return fmax(fmax(k * u0 * v0, k * u0 * v1), fmax(k * u1 * v0, k * u1 * v1));
    };
    const double tmax = corner(-2.0 * g.x, amin, amax, amin, amax) + corner(2.0 * g.y, amin, amax, bmin, bmax) +
                        corner(-2.0 * g.y, bmin, bmax, amin, amax) + corner(-2.0 * g.x, bmin, bmax, bmin, bmax);
    const cd x0 = cons[xidx & 255], x1 = cons[(xidx >> 8) & 255];
    const double lc = 2.0 * (x0.x * z0.x + x0.y * z0.y) - g00 * cabs2(x0) + 2.0 * (x1.x * z1.x + x1.y * z1.y) -
                      g11 * cabs2(x1) -
                      2.0 * (x0.x * x1.x * g.x - x0.x * x1.y * g.y + x0.y * x1.x * g.y + x0.y * x1.y * g.x);
    return (fa0 + fb0 + fa1 + fb1 + tmax - lc) * inv_s2;
}

// Column-tile bounds (column_tile_bounds) and, for NT = 4, the row-tile bound vectors of
// one symbol into its prep record `out`.
template <int NT, int NR>
__device__ __forceinline__ void prep_bounds(const cd (&H)[NT][NR], const cd (&y)[NR], double* out,
                                            const cd* cons, const PrepConst& c) {
    constexpr int NA = NT / 2, NB = NT - NA, NO = NT * NR;
    const int mask = c.M - 1;
    // ---- column-tile bounds (column_tile_bounds) ----
    {
        cd u[NA][NR];
        bool ok = true;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            cd v[NR];
            double h2 = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) { v[r] = H[q][r]; h2 += cabs2(v[r]); }
#pragma unroll
            for (int rep = 0; rep < 2; ++rep)
#pragma unroll
                for (int j = 0; j < q; ++j) {
                    cd pj = czero();
#pragma unroll
                    for (int r = 0; r < NR; ++r) pj = cfmac(pj, v[r], u[j][r]);   // u_j^H v
#pragma unroll
                    for (int r = 0; r < NR; ++r) v[r] = csub(v[r], cmul(u[j][r], pj));
                }
            double n2 = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) n2 += cabs2(v[r]);
            ok = ok && h2 > 0.0 && n2 > 1e-6 * h2;
            const double inv = ok ? fast_rsqrt(n2) : 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) u[q][r] = cscale(v[r], inv);
        }
        cd w[NR], g[NB][NR];
        double sc = 0.0, g2 = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) { w[r] = y[r]; sc += cabs2(y[r]); }
#pragma unroll
        for (int bb = 0; bb < NB; ++bb)
#pragma unroll
            for (int r = 0; r < NR; ++r) { g[bb][r] = H[NA + bb][r]; g2 += cabs2(g[bb][r]); }
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            cd pw = czero(), pg[NB];
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) pg[bb] = czero();
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                pw = cfmac(pw, w[r], u[j][r]);
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) pg[bb] = cfmac(pg[bb], g[bb][r], u[j][r]);
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                w[r] = csub(w[r], cmul(u[j][r], pw));
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) g[bb][r] = csub(g[bb][r], cmul(u[j][r], pg[bb]));
            }
        }
        double cmax2 = 0.0;
        for (int s = 0; s < c.M; ++s) cmax2 = fmax(cmax2, cabs2(cons[s]));
        out[2] = sc + NB * cmax2 * g2;
        double* lbo = out + 4 + 2 * NO;
        if (NB == 2 && c.M == 16) {
            // tile kt = first B stream b0 fixed, b1 over all 16 symbols:
            //   ||r0 - g1 x||^2 = ||r0||^2 - 2 Re(conj(x) g1^H r0) + |x|^2 ||g1||^2,
            //   r0 = w - g0 x_b0  (4 flops per hypothesis instead of NR complex products)
            double ng = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) ng += cabs2(g[NB - 1][r]);
            for (int kt = 0; kt < c.nkt; ++kt) {
                const cd xb0 = cons[kt];
                double n0 = 0.0;
                cd aa = czero();
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const cd r0 = csub(w[r], cmul(g[0][r], xb0));
                    n0 += cabs2(r0);
                    aa = cfmac(aa, r0, g[NB - 1][r]);          // g1^H r0
                }
                double lbm = INFINITY;
                for (int s1 = 0; s1 < 16; ++s1) {
                    const cd x = cons[s1];
                    const double lb = fma(cabs2(x), ng, n0 - 2.0 * (x.x * aa.x + x.y * aa.y));
                    lbm = fmin(lbm, lb);
                }
                lbo[kt] = ok ? fmax(lbm, 0.0) : 0.0;
            }
        } else
        for (int kt = 0; kt < c.nkt; ++kt) {
            double lbm = INFINITY;
            for (int s = 0; s < 16; ++s) {
                const int k = kt * 16 + s;
                double lb = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    cd res = w[r];
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb)
                        res = csub(res, cmul(g[bb][r], cons[(k >> (c.lm * (NB - 1 - bb))) & mask]));
                    lb += cabs2(res);
                }
                lbm = fmin(lbm, lb);
            }
            lbo[kt] = ok ? lbm : 0.0;
        }
    }
    // ---- row-tile bound vectors (NT = 4): the block of hypotheses with first streams
    //      (x_0, x_2) fixed has d >= ||P (y - h_0 x_0 - h_2 x_2)||^2, P = projector onto
    //      span(h_1, h_3)^perp (x_1, x_3 continuous); a degenerate basis gives P = 0 ----
    if constexpr (NT == 4) {
        cd u[2][NR];
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            cd v[NR];
            double h2 = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) { v[r] = H[2 * q + 1][r]; h2 += cabs2(v[r]); }
#pragma unroll
            for (int rep = 0; rep < 2; ++rep)
#pragma unroll
                for (int j = 0; j < q; ++j) {
                    cd pj = czero();
#pragma unroll
                    for (int r = 0; r < NR; ++r) pj = cfmac(pj, v[r], u[j][r]);
#pragma unroll
                    for (int r = 0; r < NR; ++r) v[r] = csub(v[r], cmul(u[j][r], pj));
                }
            double n2 = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) n2 += cabs2(v[r]);
            ok = ok && h2 > 0.0 && n2 > 1e-6 * h2;
            const double inv = ok ? fast_rsqrt(n2) : 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) u[q][r] = cscale(v[r], inv);
        }
        cd w[3][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) { w[0][r] = y[r]; w[1][r] = H[0][r]; w[2][r] = H[2][r]; }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                cd pw = czero();
#pragma unroll
                for (int r = 0; r < NR; ++r) pw = cfmac(pw, w[m][r], u[j][r]);
#pragma unroll
                for (int r = 0; r < NR; ++r) w[m][r] = csub(w[m][r], cmul(u[j][r], pw));
            }
        double* rbo = out + 4 + 2 * NO + ((c.nkt + 1) / 2 * 2);
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                rbo[2 * (m * NR + r)] = ok ? w[m][r].x : 0.0;
                rbo[2 * (m * NR + r) + 1] = ok ? w[m][r].y : 0.0;
            }
    }
}

// The constellation in LDS (wave-uniform loops over it read broadcasts instead of issuing a
// dependent global load per point); every thread of the block must call it.
__device__ __forceinline__ const cd* stage_cons(const cd* cons, int M) {
    __shared__ cd s_cons[64];
    if ((int)threadIdx.x < M) s_cons[threadIdx.x] = cons[threadIdx.x];
    __syncthreads();
    return s_cons;
}

template <int NT, int NR>
__global__ __launch_bounds__(256) void estep_prep_kernel(EstepArgs a, PrepConst c) {
    const cd* cons = stage_cons(a.cons, c.M);
    const long nsym = (long)c.B * c.Td;
    const long gsym = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gsym >= nsym) return;
    const int b = (int)(gsym / c.Td);
    if (a.done && a.done[b]) return;
    if (a.varn_t) {                                  // per-trial noise variance (ABI 6)
        const TrialNoise tn = trial_noise(a.varn_t[b]);
        c.reg = tn.reg; c.thr_d = tn.thr_d; c.inv_s2 = tn.inv_s2;
    }
    cd H[NT][NR];
    heff_load<NT, NR>(a, c, gsym, b, H);
    cd y[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) y[r] = a.yd[(size_t)gsym * NR + r];
    double* out = a.prep + (size_t)gsym * c.stride;
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            out[4 + 2 * (q * NR + r)] = H[q][r].x;
            out[5 + 2 * (q * NR + r)] = H[q][r].y;
        }
    cd Lm[NT][NT], zf[NT];
    double piv[NT], dinv[NT], sc;
    ridge_chol<NT, NR>(H, y, c.reg, Lm, piv, dinv, zf);
    int xidx;
    out[0] = prep_candidate<NT, NR>(H, y, Lm, dinv, zf, cons, c.M, sc, xidx);
    out[1] = sc;
    prep_bounds<NT, NR>(H, y, out, cons, c);
}

// The tile bounds of the symbols the sphere pass left to the sweep (H_eff, d0 and the scale
// are in their prep records already).  Grid over all symbols; threads past the list exit.
template <int NT, int NR>
__global__ __launch_bounds__(256) void estep_bounds_kernel(EstepArgs a, PrepConst c) {
    const long nsym = (long)c.B * c.Td;
    const long n = a.list[nsym];
    if ((long)blockIdx.x * blockDim.x >= n) return;  // the whole block is past the list
    const cd* cons = stage_cons(a.cons, c.M);
    const long gi = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n) return;
    const long gsym = a.list[gi];
    double* out = a.prep + (size_t)gsym * c.stride;
    cd H[NT][NR], y[NR];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < NR; ++r) H[q][r] = cmk(out[4 + 2 * (q * NR + r)], out[5 + 2 * (q * NR + r)]);
#pragma unroll
    for (int r = 0; r < NR; ++r) y[r] = a.yd[(size_t)gsym * NR + r];
    prep_bounds<NT, NR>(H, y, out, cons, c);
}

// ============================================================================
// Sphere pass (SPH = 1 soft, 2 hard), replacing the preparation pass when n_rx >= n_tx:
// every symbol's hypotheses inside
//   d(x) <= R,   R = R0 + 50 varn^2 (soft) / R0 (hard),   R0 = the distance of a real hypothesis,
// are enumerated exactly -- the hypotheses whose weights are not below e^-50 of the posterior
// maximum (or that can be the argmin): the set the sweep's tile bounds keep.
//   Streams are ordered by reliability (diag of (H^H H + reg I)^-1: the least reliable at
// level 0, the most reliable at the top level NT-1, as in V-BLAST).  With G' = Hp^H Hp + reg I
// = L L^H for the permuted H and zf = L^-1 Hp^H y:
//   ||y - Hp x||^2 = c0 + sum_i T_i,   c0 = ||y||^2 - ||zf||^2,
//   T_i = |L_ii x_i - e_i|^2 - reg |x_i|^2,   e_i = zf_i - sum_{j>i} conj(L_ji) x_j,
// and T_j >= -reg max|c|^2, so every hypothesis below a level-i node has
//   d - c0 >= sum_{j>=i} T_j - i reg max|c|^2.
// Distances are kept relative to c0 (common to all hypotheses of the symbol: it cancels from
// the weights and the argmin).  R0 = min(candidate, Babai point of the sorted tree).
// Part 1 (estep_tree_kernel, one THREAD per symbol): H_eff, the sweep's prep record, the
// ordering, the factorisation, the Babai point -> the symbol's tree record.
// Part 2 (estep_bfs_kernel, one WAVE per symbol): level by level, every (surviving path,
// child) pair in its own lane, survivors compacted by ballot into an LDS path list; leaves
// weighted in the lanes.  Control flow is wave-uniform: a symbol costs what its tree holds.
// A symbol whose path list outgrows `budget`, or whose G' is ill-conditioned, is listed for
// the tile bounds and the MFMA sweep.
// ============================================================================
constexpr int kTrec = kTreeRecDoubles;   // doubles per symbol of the tree record (NT <= 4)
constexpr int kBfsWaves = 4;       // waves per block of the enumeration
constexpr int kBfsSpw = 8;         // consecutive symbols per wave

template <int NT, int NR>
__global__ __launch_bounds__(256) void estep_tree_kernel(EstepArgs a, PrepConst c) {
    const cd* cons = stage_cons(a.cons, c.M);
    const long nsym = (long)c.B * c.Td;
    const long gsym = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = gsym < nsym;
    const int b = live ? (int)(gsym / c.Td) : 0;
    if (live && a.done && a.done[b]) live = false;
    if (live && a.varn_t) {                          // per-trial noise variance (ABI 6)
        const TrialNoise tn = trial_noise(a.varn_t[b]);
        c.reg = tn.reg; c.thr_d = tn.thr_d; c.inv_s2 = tn.inv_s2;
    }
    bool single = false;
    double f2d = INFINITY;            // NT = 2: the factorised pass's range bound (fact2_bound)
    if (live) {
    cd Lm[NT][NT], zf[NT];
    double piv[NT], dinv[NT], d0, sc, screen, gsum;
    int lev[NT];
    double c0 = 0.0;
    {
        cd H[NT][NR], y[NR];
        heff_load<NT, NR>(a, c, gsym, b, H);
#pragma unroll
        for (int r = 0; r < NR; ++r) y[r] = a.yd[(size_t)gsym * NR + r];
        double* out = a.prep + (size_t)gsym * c.stride;
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                out[4 + 2 * (q * NR + r)] = H[q][r].x;
                out[5 + 2 * (q * NR + r)] = H[q][r].y;
            }
        ridge_chol<NT, NR>(H, y, c.reg, Lm, piv, dinv, zf);
        int xidx;
        d0 = prep_candidate<NT, NR>(H, y, Lm, dinv, zf, cons, c.M, sc, xidx);
        out[0] = d0;
        out[1] = sc;
        screen = pair_screen<NT, NR>(H, y, xidx, cons, gsum);
        if constexpr (NT == 2)          // hard: every unresolved symbol (no exponentials, no range)
            f2d = c.pair ? (c.hard ? 0.0 : fact2_bound<NR>(H, y, xidx, cons, c.M, c.inv_s2)) : INFINITY;
        // computed here, while H and y are live anyway (left to the compiler, the computation
        // sinks to the record store at the end and keeps H_eff live across the whole kernel)
        asm volatile("" : "+v"(screen), "+v"(gsum), "+v"(f2d));
        // reliability of stream q: g_q = [(G + reg I)^-1]_qq = sum_k |(L^-1)_kq|^2
        cd W[NT][NT];
        double g[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            W[j][j] = cmk(dinv[j], 0.0);
#pragma unroll
            for (int i = j + 1; i < NT; ++i) {
                cd s = czero();
#pragma unroll
                for (int k = j; k < i; ++k) s = cfma(s, Lm[i][k], W[k][j]);
                W[i][j] = cscale(s, -dinv[i]);
            }
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            double s = 0.0;
#pragma unroll
            for (int k = q; k < NT; ++k) s += cabs2(W[k][q]);
            g[q] = s;
        }
        // level of stream q = its rank in descending g (ties by index)
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            int rk = 0;
#pragma unroll
            for (int p = 0; p < NT; ++p) rk += (g[p] > g[q] || (g[p] == g[q] && p < q)) ? 1 : 0;
            lev[q] = rk;
        }
        cd Hp[NT][NR];
#pragma unroll
        for (int l = 0; l < NT; ++l)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                cd v = H[0][r];
#pragma unroll
                for (int q = 1; q < NT; ++q) v = csel(lev[q] == l, H[q][r], v);
                Hp[l][r] = v;
            }
        ridge_chol<NT, NR>(Hp, y, c.reg, Lm, piv, dinv, zf);
#pragma unroll
        for (int r = 0; r < NR; ++r) c0 += cabs2(y[r]);
#pragma unroll
        for (int j = 0; j < NT; ++j) c0 -= cabs2(zf[j]);
    }
    double ui[NT];
    double pmin = piv[0], pmax = piv[0];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        ui[j] = piv[j] * dinv[j];                          // L_jj = sqrt(pivot)
        pmin = fmin(pmin, piv[j]);
        pmax = fmax(pmax, piv[j]);
    }
    // Babai point of the sorted tree: the nearest child level by level
    double db = 0.0, cmax2 = 0.0;
    cd xb[NT], eb[NT];
    int sb[NT];
#pragma unroll
    for (int l = NT - 1; l >= 0; --l) {
        cd e = zf[l];
#pragma unroll
        for (int j = l + 1; j < NT; ++j) e = csub(e, cmul(cconj(Lm[j][l]), xb[j]));
        const double aa = fma(ui[l], ui[l], -c.reg), m2u = -2.0 * ui[l];
        double tb = INFINITY;
        int si = 0;
        #pragma unroll 4
        for (int s = 0; s < c.M; ++s) {
            const cd x = cons[s];
            const double x2 = cabs2(x);
            cmax2 = fmax(cmax2, x2);
            const double t = fma(aa, x2, m2u * fma(x.x, e.x, x.y * e.y));
            if (t < tb) { tb = t; si = s; }
        }
        xb[l] = cons[si];
        sb[l] = si;
        eb[l] = e;
        db += tb + cabs2(e);
    }
    // ill-conditioned G': to the sweep.  So is a symbol with a pivot of G' that is the ridge alone
    // (G's own pivot is zero: a zero channel column, H_t = 0): whole classes of hypotheses are
    // at EXACTLY the same distance, the enumeration's path bounds order them by rounding
    // (aa = u^2 - reg is not 0), and only the sweep takes the first minimum in product order.
    // Only these ties are caught: exact ties that leave every pivot above the ridge (two
    // identical columns, say) are still enumerated
    const bool ok = pmax <= 1e10 * pmin && pmin > c.reg;
    const double R0 = fmin(d0 - c0, db);
    // single-path check: if along the Babai path every level has exactly one child whose
    // subtree bound is inside R (the Babai child), the Babai point is the only hypothesis
    // inside the sphere -- the posterior is x_B (weights of all others < e^-50) / the argmin
    if (ok && db <= R0) {
        const double R = R0 + (c.hard ? 0.0 : c.thr_d) + 1e-9 * sc;
        const double slack = c.reg * cmax2;
        double base = 0.0;
        bool one = true;
#pragma unroll
        for (int l = NT - 1; l >= 0; --l) {
            const cd e = eb[l];
            const double aa = fma(ui[l], ui[l], -c.reg), m2u = -2.0 * ui[l];
            const double thr = R + l * slack - base - cabs2(e);
            int n = 0;
            #pragma unroll 4
            for (int s = 0; s < c.M; ++s) {
                const cd x = cons[s];
                n += fma(aa, cabs2(x), m2u * fma(x.x, e.x, x.y * e.y)) <= thr ? 1 : 0;
            }
            one = one && n == 1;
            const cd x = xb[l];
            base += fma(aa, cabs2(x), m2u * fma(x.x, e.x, x.y * e.y)) + cabs2(e);
        }
        if (one) {
            single = true;
            constexpr int MS = NT + NT * NT;
            cd xo[NT];                                   // stream order
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                cd v = xb[0];
#pragma unroll
                for (int l = 1; l < NT; ++l) v = csel(lev[q] == l, xb[l], v);
                xo[q] = v;
            }
            cd* mo = a.mom + (size_t)gsym * MS;
            const bool arm = a.mchg != nullptr;          // the moment-repeat fold
            unsigned chg = 0;
#pragma unroll
            for (int p2 = 0; p2 < NT; ++p2) {
                mom_store(mo + p2, mom_word(xo[p2]), arm, chg);
#pragma unroll
                for (int q = 0; q < NT; ++q)
                    mom_store(mo + NT + p2 * NT + q, mom_word(cmulc(xo[p2], xo[q])), arm, chg);
            }
            if (chg) a.mchg[gsym / c.Td] = 1;            // (b is not kept live this far)
        }
    }
    // the tree record: only the enumeration reads it (not the single-path symbols, nor the
    // n_tx = 2 symbols of the factorised passes)
    if (!single && !(NT == 2 && c.pair)) {
    int packed = ok ? (1 << 16) : 0;
#pragma unroll
    for (int q = 0; q < NT; ++q) packed |= q << (4 * lev[q]);   // level l holds stream perm[l]
    double* rec = a.tree + (size_t)gsym * kTrec;
    rec[0] = c0;
    rec[1] = R0;
    rec[2] = sc;
    rec[3] = (double)packed;
    rec[kTrec - 1] = fma(gsum, cmax2, screen) * c.inv_s2;   // the pass's range bound
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        rec[4 + j] = ui[j];
        rec[4 + NT + 2 * j] = zf[j].x;
        rec[5 + NT + 2 * j] = zf[j].y;
    }
    int k = 0;
#pragma unroll
    for (int i = 1; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) {
            rec[4 + 3 * NT + 2 * k] = Lm[i][j].x;
            rec[5 + 3 * NT + 2 * k] = Lm[i][j].y;
            ++k;
        }
    }   // enumerated
    }   // live
    const bool f2 = NT == 2 && c.pair && live && !single;
    const bool wide = f2d <= kPairDmax;
    const bool enumer = live && !single && !f2;
    const int lane = threadIdx.x & 63;
    int32_t* cnt = a.list + nsym;
    // one atomic per BLOCK and list (4096 per-wave same-address atomics serialise at the L2):
    // the waves' counts through LDS, thread l reserves list l's block range
    __shared__ int s_n[2][4];
    __shared__ int s_b[2];
    const int wv = threadIdx.x >> 6;
    const unsigned long long bf = __ballot(f2 && wide), be = __ballot(enumer || (f2 && !wide));
    if (lane == 0) {
        s_n[0][wv] = __builtin_popcountll(bf);
        s_n[1][wv] = __builtin_popcountll(be);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int l = threadIdx.x;
        const int tot = s_n[l][0] + s_n[l][1] + s_n[l][2] + s_n[l][3];
        s_b[l] = tot ? atomicAdd(cnt + (l ? 2 : 3), tot) : 0;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (f2 || enumer) {
        // NT = 2 (pair mode): a symbol the factorised tables can represent (D within range; hard:
        // f2d = 0, every unresolved symbol) goes to the pair list (counter 3), a narrow one to
        // the enumeration list's slots (counter 2: no n_tx = 2 symbol is enumerated in pair mode,
        // and the enumeration is not launched) for estep_soft2_kernel; otherwise the live
        // unresolved symbols go to the enumeration list
        const bool p0 = f2 && wide;
        const int l = p0 ? 0 : 1;
        int base = s_b[l] + __builtin_popcountll((p0 ? bf : be) & lt);
        for (int w = 0; w < wv; ++w) base += s_n[l][w];
        if (p0) a.list[2 * nsym + 2 * kEstepListCnt + base] = (int32_t)gsym;
        else cnt[kEstepListCnt + base] = (int32_t)gsym;
    }
    if (c.count) {
        const unsigned long long one = __ballot(single);
        if (lane == 0) atomicAdd(&g_estep_sphere[2], (unsigned long long)__builtin_popcountll(one));
    }
}

template <int NT, int SPH>
__global__ __launch_bounds__(64 * kBfsWaves) void estep_bfs_kernel(EstepArgs a, PrepConst c) {
    typedef unsigned long long u64;
    constexpr int NP = NT * (NT - 1) / 2;
    constexpr int MS = NT + NT * NT;
    __shared__ cd s_cons[64];
    __shared__ double s_c2[64];
    __shared__ double s_pb[kBfsWaves][2][kBfsPmax];     // path bound (relative distance so far)
    __shared__ int s_pi[kBfsWaves][2][kBfsPmax];        // path symbols, level l at bits lm*l
    if ((int)threadIdx.x < c.M) {
        const cd x = a.cons[threadIdx.x];
        s_cons[threadIdx.x] = x;
        s_c2[threadIdx.x] = cabs2(x);
    }
    __syncthreads();
    double cmax2 = 0.0;
    for (int s = 0; s < c.M; ++s) cmax2 = fmax(cmax2, s_c2[s]);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long nsym = (long)c.B * c.Td;
    // the tree pass's enumeration list: wave w takes entries w*spw .. (w+1)*spw - 1
    const int32_t* elist = a.list + nsym + kEstepListCnt;
    const long nwork = __builtin_amdgcn_readfirstlane(a.list[nsym + 2]);
    const long g0 = ((long)blockIdx.x * kBfsWaves + wave) * kBfsSpw;
    if (g0 >= nwork) return;
    const long g1 = g0 + kBfsSpw < nwork ? g0 + kBfsSpw : nwork;
    const int mask = c.M - 1, lm = c.lm;
    const int pmax = c.budget < kBfsPmax ? c.budget : kBfsPmax;
    const u64 lt = (1ull << lane) - 1ull;
    unsigned listed_mask = 0, pair_mask = 0, resolved_n = 0;
    // tree records by LDS-DMA, the next symbol's in flight while the current one is enumerated
    // (lanes 0-15 carry the record's 256 bytes; the others re-read its first 16 bytes)
    __shared__ __attribute__((aligned(16))) double s_rec[kBfsWaves][2][128];
    auto issue = [&](long gi, int buf) {
        const double* src = a.tree + (size_t)elist[gi] * kTrec + (lane < kTrec / 2 ? 2 * lane : 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)s_rec[wave][buf],
                                         16, 0, 0);
    };
    issue(g0, 0);
    for (long gi = g0; gi < g1; ++gi) {
        const long gsym = elist[gi];
        // the symbol's noise constants (per-trial variances, ABI 6); per level below: T_j >= -slack
        double thr_d = c.thr_d, inv_s2 = c.inv_s2, reg = c.reg;
        if (a.varn_t) {
            const TrialNoise tn = trial_noise(a.varn_t[gsym / c.Td]);
            thr_d = uniform_d(tn.thr_d);
            inv_s2 = uniform_d(tn.inv_s2);
            reg = uniform_d(tn.reg);
        }
        const double slack = reg * cmax2;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this symbol's record landed
        wave_sync();
        const double* rec = s_rec[wave][(gi - g0) & 1];
        if (gi + 1 < g1) issue(gi + 1, (gi + 1 - g0) & 1);
        const int packed = (int)rec[3];
        bool listed = !((packed >> 16) & 1);
        const double R0 = rec[1];
        const double margin = 1e-9 * rec[2];
        const double R = R0 + (SPH == 2 ? 0.0 : thr_d) + margin;
        double ui[NT];
        cd zf[NT], Lc[NP + 1];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            ui[j] = rec[4 + j];
            zf[j] = cmk(rec[4 + NT + 2 * j], rec[5 + NT + 2 * j]);
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) Lc[k] = cmk(rec[4 + 3 * NT + 2 * k], -rec[5 + 3 * NT + 2 * k]);  // conj
        double bd = INFINITY;            // hard: this lane's best (distance, hypothesis index)
        int bj = 0x7fffffff;
        if (lane == 0) { s_pb[wave][0][0] = 0.0; s_pi[wave][0][0] = 0; }
        wave_sync();
        int n_in = 1;                    // paths entering the level; after level 0: leaves
#pragma unroll
        for (int l = NT - 1; l >= 0; --l) {
            if (listed) break;
            const int ib = (NT - 1 - l) & 1;
            const double* pbi = s_pb[wave][ib];
            const int* pii = s_pi[wave][ib];
            double* pbo = s_pb[wave][ib ^ 1];
            int* pio = s_pi[wave][ib ^ 1];
            const double u = ui[l];
            const double aa = fma(u, u, -reg), m2u = -2.0 * u;
            const double lim = R + l * slack;
            const int total = n_in << lm;
            int n_out = 0;
            for (int base = 0; base < total; base += 64) {
                const int i = base + lane;
                const bool valid = i < total;
                const int p = valid ? i >> lm : 0;
                const int s = i & mask;
                const double bp = pbi[p];
                const int ip = pii[p];
                cd e = zf[l];
#pragma unroll
                for (int j = l + 1; j < NT; ++j)      // L_jl at row-major strict index j(j-1)/2 + l
                    e = csub(e, cmul(Lc[j * (j - 1) / 2 + l], s_cons[(ip >> (lm * j)) & mask]));
                const cd x = s_cons[s];
                const double bb = bp + fma(aa, s_c2[s], m2u * fma(x.x, e.x, x.y * e.y)) + cabs2(e);
                const bool keep = valid && bb <= lim;
                const int idx = ip | (s << (lm * l));
                if (SPH == 2 && l == 0) {
                    if (keep) {
                        int jr = 0;                   // hypothesis index, original stream order
#pragma unroll
                        for (int q = 0; q < NT; ++q)
                            jr |= ((idx >> (lm * q)) & mask) << (lm * (NT - 1 - ((packed >> (4 * q)) & 15)));
                        if (bb < bd || (bb == bd && jr < bj)) { bd = bb; bj = jr; }
                    }
                } else {
                    // surviving paths (l > 0) / leaves inside the sphere (l == 0, soft)
                    const u64 bal = __ballot(keep);
                    const int slot = n_out + __builtin_popcountll(bal & lt);
                    if (keep && slot < pmax) { pbo[slot] = bb; pio[slot] = idx; }
                    n_out += __builtin_popcountll(bal);
                }
            }
            if (SPH == 2 && l == 0) break;
            if (n_out > pmax || n_out == 0) listed = true;    // too wide (or rounding lost all)
            n_in = n_out;
            wave_sync();
        }
        cd* mo = a.mom + (size_t)gsym * MS;
        if (!listed) {
            if constexpr (SPH == 2) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double od = shfl_xor_d(bd, off);
                    const int oj = __shfl_xor(bj, off);
                    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
                }
                if (bj == 0x7fffffff) listed = true;
                else if (lane < MS) {
                    const int p2 = lane < NT ? lane : (lane - NT) / NT;
                    const int q = lane < NT ? 0 : (lane - NT) % NT;
                    const cd xp = s_cons[(bj >> (lm * (NT - 1 - p2))) & mask];
                    const cd xq = s_cons[(bj >> (lm * (NT - 1 - q))) & mask];
                    unsigned chg = 0;                  // the moment-repeat fold
                    mom_store(mo + lane, mom_word(lane < NT ? xp : cmulc(xp, xq)),
                              a.mchg != nullptr, chg);
                    if (chg) a.mchg[gsym / c.Td] = 1;
                }
            } else {
                // the n_in leaves inside the sphere (LDS list, level order): lane o < MS forms
                // output o (m_t, then S_t row-major, stream order) over the list, weights
                // exp(-(d - d_min)/varn^2) for the leaves within 50 varn^2 of the minimum
                const int ib = NT & 1;
                const double* lb = s_pb[wave][ib];
                const int* li = s_pi[wave][ib];
                // every leaf's weight lane-parallel (to the free half of the path-bound buffer);
                // the output lanes then only accumulate.  The minimum stays a serial LDS scan
                // (independent reads; a 6-step cross-lane reduction costs more for the few
                // leaves most symbols have)
                double dmin = INFINITY;
                for (int k = 0; k < n_in; ++k) dmin = fmin(dmin, lb[k]);
                double* lw = s_pb[wave][ib ^ 1];
                for (int k = lane; k < n_in; k += 64) {
                    const double d = lb[k];
                    lw[k] = d <= dmin + thr_d ? fexp_neg((dmin - d) * inv_s2) : 0.0;
                }
                wave_sync();
                if (lane < MS) {
                    const int sp_ = lane < NT ? lane : (lane - NT) / NT;   // output stream pair
                    const int sq_ = lane < NT ? 0 : (lane - NT) % NT;
                    int lp = 0, lq = 0;                                    // their levels
#pragma unroll
                    for (int l = 0; l < NT; ++l) {
                        const int st = (packed >> (4 * l)) & 15;
                        lp = st == sp_ ? l : lp;
                        lq = st == sq_ ? l : lq;
                    }
                    // the moment-repeat fold: the word this lane overwrites, loaded ahead of the
                    // leaf loop
                    const bool arm = a.mchg != nullptr;
                    cd mold = czero();
                    if (arm) mold = mo[lane];
                    double z = 0.0;
                    cd v = czero();
                    for (int k = 0; k < n_in; ++k) {
                        const double w = lw[k];             // > 0 exactly for the leaves within
                        if (w != 0.0) {                     // 50 varn^2 of the minimum
                            const int id = li[k];
                            const cd xp = s_cons[(id >> (lm * lp)) & mask];
                            const cd xq = s_cons[(id >> (lm * lq)) & mask];
                            z += w;
                            v = caxpy(v, w, lane < NT ? xp : cmulc(xp, xq));
                        }
                    }
                    const cd mv = mom_word(cscale(v, 1.0 / z));
                    mo[lane] = mv;
                    if (arm && mom_bits_differ(mold, mv)) a.mchg[gsym / c.Td] = 1;
                }
            }
        }
        // a listed symbol whose range bound admits the factorised-weight pass goes to that pass
        const bool to_pair = listed && c.pair && rec[kTrec - 1] <= kPairDmax;
        wave_sync();
        if (to_pair) pair_mask |= 1u << (gi - g0);
        else if (listed) listed_mask |= 1u << (gi - g0);
        else ++resolved_n;
    }
    // the wave's listed symbols join the sweep's (or the factorised pass's) work list: one
    // atomic per wave and list
    auto append = [&](unsigned msk, int32_t* cntp, int32_t* lst) {
        const int n = __builtin_popcount(msk);
        if (!n) return;
        int base = 0;
        if (lane == 0) base = atomicAdd(cntp, n);
        base = __shfl(base, 0);
        if (lane < kBfsSpw && ((msk >> lane) & 1))
            lst[base + __builtin_popcount(msk & ((1u << lane) - 1u))] = elist[g0 + lane];
    };
    append(listed_mask, a.list + nsym, a.list);
    append(pair_mask, a.list + nsym + 3, a.list + 2 * nsym + 2 * kEstepListCnt);
    const int nl = __builtin_popcount(listed_mask) + __builtin_popcount(pair_mask);
    if (c.count && lane == 0) {
        atomicAdd(&g_estep_sphere[0], (unsigned long long)resolved_n);
        atomicAdd(&g_estep_sphere[1], (unsigned long long)nl);
    }
}

// The passes' constants, from the sweep's own geometry
PrepConst make_prep(const Problem& pb, const SweepPlan& sp, int mode) {
    PrepConst pc;
    pc.B = pb.B; pc.Td = pb.Td; pc.P = pb.P; pc.M = pb.M; pc.lm = sp.lm;
    pc.nkt = sp.JB >> 4; pc.stride = sp.prep_stride; pc.reg = sp.reg;
    pc.uni = 1;
    pc.budget = g_debug.sphere_budget;                  // path list cap per level
    pc.count = sp.count;
    pc.inv_s2 = sp.inv_s2;
    pc.thr_d = sp.thr_d;
    pc.hard = mode == SBCE_ESTEP_HARD;
    pc.pair = estep_pair_supported(pb, mode) ? 1 : 0;
    return pc;
}

}  // namespace

hipError_t estep_debug_sphere(unsigned long long* out3, int reset) {
    if (reset) {
        const unsigned long long z[3] = {0, 0, 0};
        return hipMemcpyToSymbol(HIP_SYMBOL(g_estep_sphere), z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return hipMemcpyFromSymbol(out3, HIP_SYMBOL(g_estep_sphere), 3 * sizeof(*out3), 0,
                               hipMemcpyDeviceToHost);
}

hipError_t launch_estep_prep(const Problem& pb, const EstepArgs& a, const SweepPlan& sp, int mode,
                             hipStream_t s) {
    const PrepConst pc = make_prep(pb, sp, mode);
    const long nsym = (long)pb.B * pb.Td;
    const dim3 pg((unsigned)((nsym + 255) / 256)), pblk(256);
    switch (pb.NT * 16 + pb.NR) {
#define SBCE_PREP(nt, nr) case nt * 16 + nr: hipLaunchKernelGGL((estep_prep_kernel<nt, nr>), pg, pblk, 0, s, a, pc); return hipGetLastError();
        SBCE_PREP(2, 1) SBCE_PREP(2, 2) SBCE_PREP(2, 3) SBCE_PREP(2, 4)
        SBCE_PREP(2, 5) SBCE_PREP(2, 6) SBCE_PREP(2, 7) SBCE_PREP(2, 8)
        SBCE_PREP(3, 1) SBCE_PREP(3, 2) SBCE_PREP(3, 3) SBCE_PREP(3, 4)
        SBCE_PREP(3, 5) SBCE_PREP(3, 6) SBCE_PREP(3, 7) SBCE_PREP(3, 8)
        SBCE_PREP(4, 1) SBCE_PREP(4, 2) SBCE_PREP(4, 3) SBCE_PREP(4, 4)
        SBCE_PREP(4, 5) SBCE_PREP(4, 6) SBCE_PREP(4, 7) SBCE_PREP(4, 8)
#undef SBCE_PREP
    }
    return hipErrorInvalidValue;
}

// Sphere pass (tree records, enumeration), then the tile bounds of the listed.  n_rx < n_tx
// (singular H^H H) always leaves the symbol to the sweep: not compiled
hipError_t launch_estep_sphere(const Problem& pb, const EstepArgs& a, const SweepPlan& sp, int mode,
                               hipStream_t s) {
    const PrepConst pc = make_prep(pb, sp, mode);
    const long nsym = (long)pb.B * pb.Td;
    if (!a.lists_zeroed) {
        const hipError_t me = hipMemsetAsync(a.list + nsym, 0, 5 * sizeof(int32_t), s);
        if (me != hipSuccess) return me;
    }
    const dim3 pg((unsigned)((nsym + 255) / 256)), pblk(256);
    const long nbfs = (nsym + kBfsSpw * kBfsWaves - 1) / (kBfsSpw * kBfsWaves);
    const dim3 bg((unsigned)nbfs), bblk(64 * kBfsWaves);
    const bool hard = mode == SBCE_ESTEP_HARD;
    hipError_t e;
    switch (pb.NT * 16 + pb.NR) {
// launch_estep_pair: wide posteriors of the cfg-1 geometry.  The factorised-weight pass resolves
// the symbols the enumeration routed to it and lists the ones it cannot represent for the tile
// bounds and the sweep
#define SBCE_SPH(nt, nr) case nt * 16 + nr: \
    hipLaunchKernelGGL((estep_tree_kernel<nt, nr>), pg, pblk, 0, s, a, pc); \
    if (nt == 2 && pc.pair) {} /* no enumeration: the pair passes take every listed symbol */ \
    else if (hard) hipLaunchKernelGGL((estep_bfs_kernel<nt, 2>), bg, bblk, 0, s, a, pc); \
    else hipLaunchKernelGGL((estep_bfs_kernel<nt, 1>), bg, bblk, 0, s, a, pc); \
    e = hipGetLastError(); \
    if (e == hipSuccess && pc.pair) e = launch_estep_pair(pb, a, sp.prep_stride, sp.count, mode, s); \
    if (e != hipSuccess) return e; \
    hipLaunchKernelGGL((estep_bounds_kernel<nt, nr>), pg, pblk, 0, s, a, pc); \
    return hipGetLastError();
        SBCE_SPH(2, 2) SBCE_SPH(2, 3) SBCE_SPH(2, 4) SBCE_SPH(2, 5)
        SBCE_SPH(2, 6) SBCE_SPH(2, 7) SBCE_SPH(2, 8)
        SBCE_SPH(3, 3) SBCE_SPH(3, 4) SBCE_SPH(3, 5) SBCE_SPH(3, 6) SBCE_SPH(3, 7)
        SBCE_SPH(3, 8)
        SBCE_SPH(4, 4) SBCE_SPH(4, 5) SBCE_SPH(4, 6) SBCE_SPH(4, 7) SBCE_SPH(4, 8)
#undef SBCE_SPH
    }
    return hipErrorInvalidValue;
}

}  // namespace sbce
