// Device code of expectation propagation (EP; Cespedes et al., IEEE Trans. Commun. 2014) shared by
// the EP E-steps (estep_linear.hip, SBCE_ESTEP_EP) and the EP kind of the linear soft detector
// (detect_linear.hip, SBCE_LINEAR_EP); DESIGN.md §3.13.  EP loops the LMMSE solve of
// linear_solve.h, each pass using the per-stream posterior means and variances of the pass before
// as a Gaussian prior.  Per symbol, with G = H^H H, u = H^H y, s2 the posterior denominator and
// es the mean symbol energy, the state of stream a is r_a (real) and q_a (complex) -- s2 lambda_a
// and s2 gamma_a of the paper -- starting at r_a = s2 / es, q_a = 0.  Pass l = 1..p:
//   1. A = G + diag(r) = L L^H (a pivot <= 1e-14 max_a A_aa fails the symbol)
//   2. g_a = (A^-1)_aa,  z = A^-1 (u + q)
//   3. mu_a = 1 - r_a g_a;  cavity variance h2_a = s2 g_a / mu_a;  cavity mean
//      t_a = (z_a - g_a q_a) / mu_a
//   4. demap on (t_a, h2_a) (lin_demap): weights e^{-(|t_a - cons[s]|^2 - d_min) / h2_a},
//      m_a = sum post cons,  s_a = sum post |cons|^2
//   5. l = p: stop.  Else v_a = max(s_a - |m_a|^2, kEpVarFloor es),  r' = s2 (1 / v_a - 1 / h2_a),
//      q' = s2 (m_a / v_a - t_a / h2_a);  r' finite and > 0: r_a <- beta r' + (1 - beta) r_a and
//      q_a likewise (beta = kEpBeta);  otherwise both keep their values.
// Pass 1 is the MMSE solve of linear_solve.h (rho = s2 / es on every lane, q = 0 adds an exact
// zero) up to rounding: p = 1 gives lin_solve + lin_estimate's x_soft and nu within their bound.
// Degenerate cases: a failed pivot in any pass makes every stream of the symbol dead in that pass
// and in the last one (t = 0, h2 = +inf: the uniform posterior); a stream with mu_a <= 0 in a pass
// is dead for itself in that pass; a dead stream keeps its r and q.
// Work split: the group of 8 lanes of a symbol, lane a = column a, as lin_solve.  Column a of G
// and conj(u_a) (NT + 1 complex) are formed ONCE from LDS and stay in registers across the passes.
// Every sum's order is fixed by (NT, NR, M, p) alone; cross-lane moves only copy.
#pragma once

#include "linear_solve.h"

namespace sbce {

constexpr double kEpBeta = 0.5;          // damping of the state update
constexpr double kEpVarFloor = 5e-7;     // floor of the posterior variance, in units of es
// kEpDefaultPasses, kEpMaxPasses and ep_passes_of(): sbce_internal.h (the entry points read them)

// Column aa of G = H^H H in c0[0..NT-1] and conj(u_aa) in c0[NT]: lin_solve's sums, term for term.
template <int NT>
__device__ __forceinline__ void ep_gram(const cd* Hs, const cd* y, int NR, int aa, cd (&c0)[NT + 1]) {
#pragma unroll
    for (int i = 0; i <= NT; ++i) c0[i] = czero();
    for (int r = 0; r < NR; ++r) {
        const cd ha = Hs[aa * NR + r];
#pragma unroll
        for (int i = 0; i < NT; ++i) c0[i] = cfmac(c0[i], ha, Hs[i * NR + r]);
        c0[NT] = cfmac(c0[NT], ha, y[r]);
    }
}

// One solve: A = G + diag(r) (this lane adds its own r to its diagonal entry), right-hand side
// u + q.  Out: g = (A^-1)_aa, z = (A^-1 (u + q))_aa, fail (the whole group agrees on it).
// lin_solve's right-looking Cholesky with its folded forward substitution L w = e_a, in half the
// registers -- which the copy of G's column kept across the passes needs at n_tx = 8.  In lane a
// the column entries c[i] matter only until step a (lane a broadcasts column a at step a; its
// entries j < a give L[a][j] = conj(c[j]) / sqrt(piv_j), the Schur complement being Hermitian) and
// w[i] is zero until step a, so ONE array x holds c before step a and w from step a on.  Both
// updates are x[i] -= l_ij * (x[j] / sqrt(piv_j)): conj(L[a][j]) before step a, w_j after it; at
// step a itself w_a = 1 and x[i > a] restarts from 0 once it has been broadcast.
template <int NT>
__device__ __forceinline__ void ep_solve(const cd (&c0)[NT + 1], double r, cd q, int aa, int lane,
                                         double& g, cd& z, bool& fail) {
    cd x[NT + 1];
    double diag = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const bool d = i == aa;
        x[i] = c0[i];
        x[i].x = d ? x[i].x + r : x[i].x;
        diag = d ? x[i].x : diag;
    }
    x[NT] = cmk(c0[NT].x + q.x, c0[NT].y - q.y);        // conj((u + q)_a)
    const double tol = 1e-14 * group8_max(diag);

    fail = false;
    g = 0.0;
    z = czero();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int addr = ((lane & 56) | j) << 2;
        const double piv = bperm_d(x[j].x, addr);       // lane j still holds c[j] at step j
        fail = fail || !(piv > tol);
        const double rinv = fast_rsqrt64(piv);
        const bool own = j == aa;
        const cd mult = cscale(csel(own, cmk(1.0, 0.0), x[j]), rinv);
        const cd wj = csel(aa > j, czero(), mult);
        g = fma(wj.x, wj.x, g);
        g = fma(wj.y, wj.y, g);
#pragma unroll
        for (int i = j + 1; i <= NT; ++i) {
            const cd lji = cscale(bperm_c(x[i], addr), rinv);
            if (i == NT) z = cfmac(z, cconj(wj), lji);  // conj(w_j) u_j, u_j = conj(lji)
            x[i] = cfma(csel(own, czero(), x[i]), cmk(-lji.x, -lji.y), mult);
        }
    }
}

// The cavity of stream a: mean t, variance h2 and inv = 1 / h2; a dead stream (failed symbol or
// mu <= 0) gets t = 0, h2 = +inf, inv = 0 as lin_estimate gives it.
__device__ __forceinline__ void ep_cavity(double r, cd q, double s2, double g, cd z, bool fail,
                                          cd& t, double& h2, double& inv, bool& dead) {
    const double mu = fma(-r, g, 1.0);
    const double rmu = 1.0 / mu;
    t = cscale(cmk(fma(-g, q.x, z.x), fma(-g, q.y, z.y)), rmu);
    h2 = s2 * g;
    h2 *= rmu;
    dead = !(mu > 0.0) || fail;
    if (dead) {
        t = czero();
        h2 = INFINITY;
    }
    inv = dead ? 0.0 : 1.0 / h2;
}

// The pass loop from the state (r, q): solve, cavity, and between two passes the demapper's moments
// and the damped update of step 5.  demap(t, inv, mean, saa) is the kind's demapper (the plain one,
// or the one that carries the a-priori pmf).  Out: the cavity (t, h2, inv) of the last pass, dead =
// this stream is dead in it, fail = a pivot failed in some pass (the whole group agrees; every
// stream is then dead).
template <int NT, class Demap>
__device__ __forceinline__ void ep_passes(const cd (&c0)[NT + 1], double r, cd q, double s2,
                                          double es, int passes, int aa, int lane, Demap demap,
                                          cd& t, double& h2, double& inv, bool& dead, bool& fail) {
    const double vfloor = kEpVarFloor * es;
    fail = false;
    for (int l = 1;; ++l) {
        double g;
        cd z;
        bool f;
        ep_solve<NT>(c0, r, q, aa, lane, g, z, f);
        fail = fail || f;
        ep_cavity(r, q, s2, g, z, fail, t, h2, inv, dead);
        if (l >= passes) break;
        cd mean;
        double saa;
        demap(t, inv, mean, saa);
        const double v = fmax(saa - cabs2(mean), vfloor);
        const double iv = 1.0 / v;
        const double rn = s2 * (iv - inv);
        const cd qn = cmk(s2 * (mean.x * iv - t.x * inv), s2 * (mean.y * iv - t.y * inv));
        const bool up = !dead && rn > 0.0 && rn < INFINITY;
        r = up ? kEpBeta * rn + (1.0 - kEpBeta) * r : r;
        q = csel(up, cmk(kEpBeta * qn.x + (1.0 - kEpBeta) * q.x, kEpBeta * qn.y + (1.0 - kEpBeta) * q.y), q);
    }
}

// `passes` passes from the uniform pmf's state (r = s2 / es, q = 0) with the plain demapper
// (lin_demap), on G's column and conj(u) in c0.
template <int NT>
__device__ __forceinline__ void ep_run(const cd (&c0)[NT + 1], const cd* cons_s, int M, double s2,
                                       double es, int passes, int aa, int lane, cd& t, double& h2,
                                       double& inv, bool& fail) {
    bool dead;
    ep_passes<NT>(
        c0, s2 / es, czero(), s2, es, passes, aa, lane,
        [&](cd tc, double ic, cd& mc, double& sc) { lin_demap(cons_s, M, tc, ic, mc, sc); }, t, h2,
        inv, dead, fail);
}

}  // namespace sbce
