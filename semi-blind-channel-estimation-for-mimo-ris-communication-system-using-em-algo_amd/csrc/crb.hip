// Cramer-Rao bound / predicted error variance (sbce_crb): diag(R^-1) and tr(R^-1) of every trial's
// normal matrix R (L <= 512), from the lower triangle the M-step's build leaves in the workspace.
//
// One 4-wave workgroup per trial, 16 x 16 complex tiles, T = ceil(L / 16) tile rows; R is worked on
// in place (global memory, a trial's R stays in L2), LDS holds one diagonal-tile inverse, one
// scratch tile per wave and the L row sums.
//   1. R = G G^H, left-looking by tile column j.  (a) every tile (i, j), i >= j, takes its update
//      - sum_{k<j} G_ik G_jk^H (MFMA; tile rows dealt to the waves); the wave that holds (j, j)
//      factors it in LDS (v_rsq_f64 + Newton pivots) and inverts the factor, D_j = G_jj^-1, to LDS
//      and to the scratch.  (b) G_ij = A_ij D_j^H (MFMA).  One barrier after each half.
//   2. W = G^-1, kept as U = W^H in R's strict upper tiles: for tile row j of U (dealt to the waves,
//      no barrier: row j reads G, the D tiles and its own earlier tiles only)
//        U_ji = - (sum_{k=j}^{i-1} G_ik U_jk^H)^H D_i^H,   U_jj = D_j^H  (read from the scratch).
//   3. diag_inv[l] = sum_{c >= l} |U_lc|^2, one wave per row (lanes strided over c, DPP sum), then
//      tr_inv = sum_l diag_inv[l] by wave 0.
// Every order of summation is a function of L alone, no atomic is used, and every element that is
// read was written by this launch or by the build: the result does not depend on the batch or on
// what the workspace held.  A ragged last tile (L not a multiple of 16) is the same code: loads
// past L give 0 (1 on the diagonal of the last diagonal tile), stores past L are dropped.
// Pivot rule (the project's): a pivot that is not above 1e-14 max_l R_ll makes the trial
// unidentifiable -- every output +inf, SBCE_STATUS_NONHPD -- and ends its work.
#include "sbce_internal.h"

namespace sbce {

namespace {

constexpr int NB = 16;
constexpr int kCrbThreads = 256;

// lane operand of tile (r0, c0) of the row-major matrix M for k-step s of C -= A T^H (A and T
// alike): element [li][4 s + lk]
__device__ __forceinline__ cd ld_op(const cd* M, int L, int r0, int c0, int s, int li, int lk) {
    const int r = r0 + li, c = c0 + 4 * s + lk;
    return (r < L && c < L) ? M[(size_t)r * L + c] : czero();
}

__device__ __forceinline__ cd cneg(cd a) { return cmk(-a.x, -a.y); }

// Cholesky factor of the Hermitian tile X (LDS, row-major, lower triangle read) in one wave, in
// place; rs[c] = 1 / G_cc.  npad: rows at or past it are identity padding (no pivot test).
// Returns true when a pivot failed the rule.
__device__ __forceinline__ bool factor_tile(cd* X, double* rs, double tol, int npad, int lane) {
    bool bad = false;
    for (int c = 0; c < NB; ++c) {
        double d = X[c * NB + c].x;
        const bool ok = d > tol || c >= npad;
        if (!ok) { bad = true; d = 1.0; }
        const double r = fast_rsqrt64(d);
        wave_sync();
        if (lane < NB) {
            if (lane > c) X[lane * NB + c] = cscale(X[lane * NB + c], r);
            if (lane == c) { X[c * NB + c] = cmk(d * r, 0.0); rs[c] = r; }
        }
        wave_sync();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int idx = lane + 64 * m, rr = idx >> 4, c2 = idx & 15;
            if (c2 > c && rr >= c2) {
                const cd v = cmulc(X[rr * NB + c], X[c2 * NB + c]);
                X[idx] = csub(X[idx], v);
            }
        }
        wave_sync();
    }
    return bad;
}

// D = G^-1 of the lower-triangular tile X (LDS) in one wave: lane c (< 16) forward-substitutes
// column c; the result goes to Dl (LDS) and Dg (global scratch), zeros above the diagonal
__device__ __forceinline__ void invert_tile(const cd* X, const double* rs, cd* Dl, cd* Dg, int lane) {
    if (lane >= NB) return;
    const int c = lane;
    // the column is kept in Dl: a lane reads back only what it wrote itself
#pragma unroll 1
    for (int r = 0; r < NB; ++r) {
        cd s = cmk(r == c ? 1.0 : 0.0, 0.0);
#pragma unroll 1
        for (int k = c; k < r; ++k) s = cfma(s, cneg(X[r * NB + k]), Dl[k * NB + c]);
        // rows above the column's diagonal are zero
        const cd x = r < c ? czero() : cscale(s, rs[r]);
        Dl[r * NB + c] = x;
        Dg[r * NB + c] = x;
    }
}

struct CrbArgs {
    cd* R;                    // [B][L][L] lower triangle in; overwritten
    cd* dinv;                 // [B][T][16][16] scratch: the diagonal tiles' inverses
    const cd* h_true;         // [B][K] or null
    const double* sigma2_t;   // [B] or null
    double sigma2;
    double* tr_inv;           // [B]
    double* diag_inv;         // [B][L] or null
    double* mse;              // [B] or null
    double* bound;            // [B] or null
    int32_t* status;          // [B] or null
};

__global__ __launch_bounds__(kCrbThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void crb_kernel(CrbArgs a, int L, int NR) {
    __shared__ cd sD[NB * NB];            // D_j of the current tile column
    __shared__ cd sW[4][NB * NB];         // one scratch tile per wave
    __shared__ double sdiag[kLargeL];     // the row sums
    __shared__ double srs[NB];
    __shared__ double red[4];
    __shared__ int sbad;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int T = (L + NB - 1) / NB;
    cd* R = a.R + (size_t)b * L * L;
    cd* Dv = a.dinv + (size_t)b * T * NB * NB;

    // ---- pivot threshold 1e-14 max_l R_ll
    double mx = 0.0;
    for (int l = tid; l < L; l += kCrbThreads) mx = fmax(mx, R[(size_t)l * L + l].x);
    mx = wave_max_dpp(mx);
    if (tid == 0) sbad = 0;
    if (lane == 0) red[w] = mx;
    __syncthreads();
    const double tol = 1e-14 * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    bool bad = false;

    // ---- 1. R = G G^H
    for (int j = 0; j < T && !bad; ++j) {
        for (int i = j + w; i < T; i += 4) {
            mf4 cre, cim, c2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {            // C layout: row lk + 4 q, column li
                const int r = NB * i + lk + 4 * q, c = NB * j + li;
                cd v = (r < L && c < L) ? R[(size_t)r * L + c] : czero();
                if (i == j && r == c && r >= L) v = cmk(1.0, 0.0);
                cre[q] = v.x; cim[q] = v.y;
            }
            csub_init<false>(cre, cim, c2);
            for (int k = 0; k < j; ++k) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    csub_step<false>(cre, cim, c2, ld_op(R, L, NB * i, NB * k, s, li, lk),
                                     ld_op(R, L, NB * j, NB * k, s, li, lk));
            }
            if (i == j) {                            // the diagonal tile: factor and invert (wave 0)
                cd* X = sW[w];
#pragma unroll
                for (int q = 0; q < 4; ++q) X[(lk + 4 * q) * NB + li] = csub_out<false>(cre, cim, c2, q);
                wave_sync();
                const bool f = factor_tile(X, srs, tol, L - NB * j, lane);
                if (f && lane == 0) sbad = 1;
                invert_tile(X, srs, sD, Dv + (size_t)j * NB * NB, lane);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int idx = lane + 64 * m, rr = idx >> 4, cc = idx & 15;
                    if (rr >= cc && NB * j + rr < L) R[(size_t)(NB * j + rr) * L + NB * j + cc] = X[idx];
                }
                wave_sync();
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = NB * i + lk + 4 * q, c = NB * j + li;
                    if (r < L) R[(size_t)r * L + c] = csub_out<false>(cre, cim, c2, q);
                }
            }
        }
        __syncthreads();
        bad = sbad != 0;
        if (!bad) {
            for (int i = j + 1 + w; i < T; i += 4) {     // G_ij = A_ij D_j^H
                mf4 cre = {0.0, 0.0, 0.0, 0.0}, cim = {0.0, 0.0, 0.0, 0.0}, c2;
                csub_init<false>(cre, cim, c2);
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    csub_step<false>(cre, cim, c2, cneg(ld_op(R, L, NB * i, NB * j, s, li, lk)),
                                     sD[li * NB + 4 * s + lk]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = NB * i + lk + 4 * q, c = NB * j + li;
                    if (r < L) R[(size_t)r * L + c] = csub_out<false>(cre, cim, c2, q);
                }
            }
        }
        __syncthreads();
    }

    if (!bad) {
        // ---- 2. U = (G^-1)^H in the strict upper tiles, tile row j by one wave
        cd* S = sW[w];
        for (int j = w; j < T; j += 4) {
            const cd* Dj = Dv + (size_t)j * NB * NB;
            for (int i = j + 1; i < T; ++i) {
                mf4 cre = {0.0, 0.0, 0.0, 0.0}, cim = {0.0, 0.0, 0.0, 0.0}, c2;
                csub_init<false>(cre, cim, c2);
                // k = j: U_jj = D_j^H, element [li][4 s + lk] = conj(D_j[4 s + lk][li])
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    csub_step<false>(cre, cim, c2, cneg(ld_op(R, L, NB * i, NB * j, s, li, lk)),
                                     cconj(Dj[(4 * s + lk) * NB + li]));
                for (int k = j + 1; k < i; ++k) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        csub_step<false>(cre, cim, c2, cneg(ld_op(R, L, NB * i, NB * k, s, li, lk)),
                                         ld_op(R, L, NB * j, NB * k, s, li, lk));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) S[(lk + 4 * q) * NB + li] = csub_out<false>(cre, cim, c2, q);
                wave_sync();
                // U_ji = - S^H D_i^H: A = S^H, element [li][4 s + lk] = conj(S[4 s + lk][li])
                const cd* Di = Dv + (size_t)i * NB * NB;
                mf4 ure = {0.0, 0.0, 0.0, 0.0}, uim = {0.0, 0.0, 0.0, 0.0}, u2;
                csub_init<false>(ure, uim, u2);
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    csub_step<false>(ure, uim, u2, cconj(S[(4 * s + lk) * NB + li]),
                                     Di[li * NB + 4 * s + lk]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = NB * j + lk + 4 * q, c = NB * i + li;
                    if (c < L) R[(size_t)r * L + c] = csub_out<false>(ure, uim, u2, q);
                }
                // the tile is read back by this wave (other lanes) at the next i
                __threadfence_block();
                wave_sync();
            }
        }
        __syncthreads();

        // ---- 3. row sums of |U|^2
        for (int l = w; l < L; l += 4) {
            const int jt = l / NB, l0 = l - NB * jt;
            const cd* Dj = Dv + (size_t)jt * NB * NB;
            double acc = 0.0;
            for (int c = NB * jt + lane; c < L; c += 64) {
                const int k = c - NB * jt;
                const cd v = k < NB ? Dj[k * NB + l0] : R[(size_t)l * L + c];
                acc += cabs2(v);
            }
            acc = wave_sum_dpp(acc);
            if (lane == 0) sdiag[l] = acc;
        }
    }
    __syncthreads();

    // ---- outputs
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    if (a.diag_inv)
        for (int l = tid; l < L; l += kCrbThreads) a.diag_inv[(size_t)b * L + l] = bad ? inf : sdiag[l];
    double hn = 0.0;
    if (a.bound) {                               // ||h_true_b||^2
        const cd* h = a.h_true + (size_t)b * L * NR;
        for (int k = tid; k < L * NR; k += kCrbThreads) hn += cabs2(h[k]);
        hn = block_sum4(wave_sum_dpp(hn), red, lane, w);
    }
    if (w == 0) {
        double tr = 0.0;
        if (!bad)
            for (int l = lane; l < L; l += 64) tr += sdiag[l];
        tr = bad ? inf : wave_sum_dpp(tr);
        if (lane == 0) {
            const double s2 = a.sigma2_t ? a.sigma2_t[b] : a.sigma2;
            const double mse = (double)NR * s2 * tr;
            a.tr_inv[b] = tr;
            if (a.mse) a.mse[b] = mse;
            if (a.bound) a.bound[b] = mse / hn;
            if (bad && a.status) a.status[b] |= SBCE_STATUS_NONHPD;
        }
    }
}

}  // namespace

size_t crb_dinv_bytes(const Problem& pb) {
    const size_t T = (size_t)(pb.L + NB - 1) / NB;
    return (size_t)pb.B * T * NB * NB * sizeof(cd);
}

hipError_t launch_crb(const Problem& pb, cd* R, cd* dinv, const cd* h_true, const sbce_crb_opts& o,
                      int32_t* status, hipStream_t s) {
    if (pb.L < 1 || pb.L > kLargeL) return hipErrorInvalidValue;
    CrbArgs a;
    a.R = R; a.dinv = dinv; a.h_true = h_true; a.sigma2_t = o.sigma2_t; a.sigma2 = o.sigma2;
    a.tr_inv = o.tr_inv; a.diag_inv = o.diag_inv; a.mse = o.mse; a.bound = o.bound; a.status = status;
    hipLaunchKernelGGL(crb_kernel, dim3(pb.B), dim3(kCrbThreads), 0, s, a, pb.L, pb.NR);
    return hipGetLastError();
}

}  // namespace sbce
