// Device code of soft-input expectation propagation (include/sbce.h sbce_detect_linear_prior,
// sbce_estep_prior), shared by the prior kind of estep_linear.hip and the prior
// kernel of detect_linear.hip.  The passes are ep_solve.h's -- the solve, the pivot rule, the
// cavity and the pass loop are ep_solve, ep_cavity and ep_passes themselves -- with two changes:
// the state starts from the moments of the a-priori pmf instead of the uniform one, and the
// demapper weighs every table point by its a-priori probability.
// The prior of stream a is given as lgM bit L-values La_i = log(P(bit_i = 0) / P(bit_i = 1)),
// sanitised on load (NaN -> 0, clamped to +-kPriorClamp), with bit_i(s) = (labels[s] >> i) & 1:
//   lp[s] = -sum_i bit_i(s) La_i - max_s(...)  =  -sum_i |La_i| [bit_i(s) != (La_i < 0)]
// -- the largest member is the point whose every bit agrees with the sign of its L-value, so the
// shift needs no pass over the table and lp <= 0 with one member 0.
// Storage: the lane keeps -|La_i| (6 doubles) and the sign bits (one int) of ITS stream in
// registers and forms lp[s] beside each exponent from labels in LDS: lgM selects and adds, no
// per-symbol table.
// Every sum's order is fixed by (NT, NR, M, p) alone; cross-lane moves only copy.
#pragma once

#include "ep_solve.h"

namespace sbce {

constexpr double kPriorClamp = 64.0;     // |La| after the load: e^-64 is the weight of a known bit

struct EpPrior {
    double pen[6];     // -|La_i|; 0 for i >= lgM
    int neg;           // bit i: La_i < 0
};

// The sanitised L-values of one stream; la points at its lgM values.
__device__ __forceinline__ EpPrior ep_prior_load(const double* la, int lgM) {
    EpPrior p;
    p.neg = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        p.pen[i] = 0.0;
        if (i < lgM) {
            double v = la[i];
            v = v != v ? 0.0 : v;
            v = fmin(fmax(v, -kPriorClamp), kPriorClamp);
            p.neg |= v < 0.0 ? 1 << i : 0;
            p.pen[i] = -fabs(v);
        }
    }
    return p;
}

// the sanitised La_i back from its two parts
__device__ __forceinline__ double ep_prior_la(const EpPrior& p, int i) {
    return (p.neg >> i) & 1 ? p.pen[i] : -p.pen[i];
}

// lp of the table point labelled lab
__device__ __forceinline__ double ep_prior_lp(const EpPrior& p, int lab, int lgM) {
    const int dis = lab ^ p.neg;
    double lp = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < lgM) lp += (dis >> i) & 1 ? p.pen[i] : 0.0;
    return lp;
}

// The exponent of table point s on the cavity (t, 1 / h2): -|t - cons[s]|^2 / h2 + lp[s].  One
// expression for every pass over the table, so that the largest exponent is met again bit for bit.
__device__ __forceinline__ double ep_prior_exponent(const EpPrior& p, cd cs, int lab, int lgM, cd t,
                                                    double inv) {
    return fma(-cabs2(csub(t, cs)), inv, ep_prior_lp(p, lab, lgM));
}

// lin_demap with the prior: weights e^{exponent - largest exponent}, posterior mean and second
// moment.  inv = 0 (a dead stream, or the call that forms the prior's own moments) leaves the
// a-priori pmf.
__device__ __forceinline__ void ep_prior_demap(const cd* cons_s, const int* lab_s, int M, int lgM,
                                               const EpPrior& p, cd t, double inv, cd& mean,
                                               double& saa) {
    double emax = -INFINITY;
    for (int s = 0; s < M; ++s)
        emax = fmax(emax, ep_prior_exponent(p, cons_s[s], lab_s[s], lgM, t, inv));
    double Z = 0.0;
    saa = 0.0;
    mean = czero();
    for (int s = 0; s < M; ++s) {
        const cd cs = cons_s[s];
        const double e = fexp_neg(ep_prior_exponent(p, cs, lab_s[s], lgM, t, inv) - emax);
        Z += e;
        mean = caxpy(mean, e, cs);
        saa = fma(e, cabs2(cs), saa);
    }
    mean = cmk(mean.x / Z, mean.y / Z);
    saa /= Z;
}

// ep_run from the prior's moments: r = s2 / v0, q = s2 xbar / v0 with xbar and v0 the mean and the
// floored variance of the a-priori pmf, and ep_prior_demap between the passes.  Out: ep_passes'.
template <int NT>
__device__ __forceinline__ void ep_prior_run(const cd (&c0)[NT + 1], const cd* cons_s,
                                             const int* lab_s, int M, int lgM, const EpPrior& p,
                                             double s2, double es, int passes, int aa, int lane,
                                             cd& t, double& h2, double& inv, bool& dead, bool& fail) {
    cd mean;
    double saa;
    ep_prior_demap(cons_s, lab_s, M, lgM, p, czero(), 0.0, mean, saa);
    const double r = s2 / fmax(saa - cabs2(mean), kEpVarFloor * es);
    ep_passes<NT>(
        c0, r, cscale(mean, r), s2, es, passes, aa, lane,
        [&](cd tc, double ic, cd& mc, double& sc) {
            ep_prior_demap(cons_s, lab_s, M, lgM, p, tc, ic, mc, sc);
        },
        t, h2, inv, dead, fail);
}

}  // namespace sbce
