// Semi-blind Gaussian-approximation EM, the comparator of "Comparision/Comparision T_d vs
// NMSE.py":106-145 (EM_approx; the same function at "Comparision/Comparision T_p .py":74-113),
// for a batch of independent trials in ONE launch: one workgroup per trial, every update of the
// trial inside the kernel.
//
// Model y_t = G^H psi_t x_t + z_t, G N x M (M = n_rx), scalar symbols.  One update from G:
//   g_t = G^H psi_t, a_t = ||g_t||^2, mu_t = g_t^H y_t / (a_t + v^2)          (:122-126)
//   q_t = (psi_t^T G)(G^H psi_t)   -- a plain transpose (:128): complex, not a_t
//   c_t = v^2 / (q_t + v^2) + |mu_t|^2                                           (:129-131)
//   A = A_p + sum_t c_t psi_t psi_t^H,  Rows = Rows_p + sum_t y_t conj(mu_t) psi_t^H
//   G_new = (Rows A^-1)^H                                                        (:140-141)
// A is complex and NOT Hermitian (c_t is complex).  The kernel builds W = A^T and the right-hand
// sides Rows^T as one augmented N x (N + M) matrix in LDS and solves W Z = Rows^T by Gauss-Jordan
// elimination with partial pivoting; G_new = conj(Z).
//
// Work split of the 256 threads (4 waves):
//   per-symbol stage  one wave per symbol; lane = (m, n mod 8) holds G[n][m] for its 8 rows in
//                     registers, psi_t streams from global memory; butterfly sums over n, then m
//   W / rhs build     thread (ti, tj) of a 16 x 16 grid owns W[ti + 16 a][tj + 16 b], a, b < R =
//                     ceil(N / 16), in registers (the pilot part A_p, Rows_p is kept in a second
//                     register set for the whole call); two rhs entries per thread
//   solve             rows over threads, one barrier per pivot column
// Every sum has a fixed order and nothing is shared between workgroups: a trial's result does
// not depend on the batch around it.
#include "sbce_internal.h"

namespace sbce {

namespace {

constexpr int kApxThreads = 256;
constexpr int kApxChunk = 64;      // data symbols between two barriers of an update
constexpr int kApxMaxN = 64;
constexpr int kApxMaxM = 8;

// 1 / x from v_rcp_f64 and two Newton steps
__device__ __forceinline__ double fast_rcp64(double x) {
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}

__device__ __forceinline__ cd shfl_xor_c(cd v, int m) {
    return cmk(shfl_xor_d(v.x, m), shfl_xor_d(v.y, m));
}

// p[i] for i < n, else 0: the load itself is unconditional (index clamped into the row, n >= 1),
// so a guarded element costs a select, not a branch
__device__ __forceinline__ cd ld_or_zero(const cd* p, int i, int n) {
    const cd v = p[i < n ? i : 0];
    return csel(i < n, v, czero());
}

__host__ __device__ inline int apx_ld(int N, int M) { return (N + M) | 1; }   // odd row stride

template <int R>
__global__ __launch_bounds__(kApxThreads) void approx_em_kernel(ApproxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, M = a.M, Tp = a.Tp, Td = a.Td;
    const int LD = apx_ld(N, M);
    cd* W = (cd*)smem;                              // [N][LD]: W = A^T | Rows^T
    cd* Gs = W + (size_t)N * LD;                    // [N][M]   the new G, handed to every wave
    cd* cmu = Gs + (size_t)N * M;                   // [2][kApxChunk][2]: c_t, conj(mu_t)
    int* piv = (int*)(cmu + 2 * kApxChunk * 2);     // [N] pivot row of each column

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const cd* yd = a.yd + (size_t)b * Td * M;
    const cd* yp = a.yp + (size_t)b * Tp * M;
    const cd* psid = a.psid + (size_t)b * Td * N;
    const cd* psip = a.psip + (size_t)b * Tp * N;
    const cd* xp = a.xp + (size_t)b * Tp;
    cd* g = a.g + (size_t)b * N * M;
    const double v = a.varn_t ? a.varn_t[b] : a.varn;
    const double v2 = v * v;

    // ---- ownership
    const int ti = tid >> 4, tj = tid & 15;         // W tile grid
    int en[2], em[2];                               // rhs entries (n, m); n = -1: none
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = tid + k * kApxThreads;
        en[k] = e < N * M ? e / M : -1;
        em[k] = e < N * M ? e % M : 0;
    }
    const int ml = lane & 7, ns = lane >> 3;        // per-symbol stage: column m, rows ns + 8 i

    // ---- once per trial: the pilot parts, W_p = A_p^T and Rows_p^T
    cd accP[R][R], rP[2];
#pragma unroll
    for (int x = 0; x < R; ++x)
#pragma unroll
        for (int y = 0; y < R; ++y) accP[x][y] = czero();
    rP[0] = rP[1] = czero();
    for (int p = 0; p < Tp; ++p) {
        const cd x = xp[p];
        const double w = cabs2(x);
        const cd* ps = psip + (size_t)p * N;
        cd pj[R];
#pragma unroll
        for (int y = 0; y < R; ++y) pj[y] = ld_or_zero(ps, tj + 16 * y, N);
#pragma unroll
        for (int x2 = 0; x2 < R; ++x2) {
            const cd wi = cscale(cconj(ld_or_zero(ps, ti + 16 * x2, N)), w);
#pragma unroll
            for (int y = 0; y < R; ++y) accP[x2][y] = cfma(accP[x2][y], wi, pj[y]);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (en[k] >= 0) rP[k] = cfmac(rP[k], cmulc(yp[(size_t)p * M + em[k]], x), ps[en[k]]);
    }

    // ---- G_0 into the per-symbol stage's registers
    cd greg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = ns + 8 * i;
        greg[i] = (ml < M && n < N) ? g[(size_t)n * M + ml] : czero();
    }

    const int npad = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
    const int tpr = kApxThreads / npad;             // threads per row of the elimination
    const int gi = tid / tpr, gc = tid % tpr;
    bool singular = false;
    int buf = 0;

    for (int it = 0; it < a.iters; ++it) {
        cd acc[R][R], rr[2];
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) acc[x][y] = accP[x][y];
        rr[0] = rP[0];
        rr[1] = rP[1];

        for (int c0 = 0; c0 < Td; c0 += kApxChunk, buf ^= 1) {
            const int nc = Td - c0 < kApxChunk ? Td - c0 : kApxChunk;
            cd* cm = cmu + buf * kApxChunk * 2;
            // per-symbol stage: conditional mean and variance of the chunk's symbols
            for (int tt = wave; tt < nc; tt += kApxThreads / 64) {
                const int t = c0 + tt;
                const cd* ps = psid + (size_t)t * N;
                cd gs = czero(), ss = czero();
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int n = ns + 8 * i;
                    const cd p = ld_or_zero(ps, n, N);
                    gs = cfmac(gs, p, greg[i]);     // conj(G[n][m]) psi_n
                    ss = cfma(ss, p, greg[i]);      // G[n][m] psi_n
                }
#pragma unroll
                for (int off = 8; off < 64; off <<= 1) {
                    gs = cadd(gs, shfl_xor_c(gs, off));
                    ss = cadd(ss, shfl_xor_c(ss, off));
                }
                const cd y = ld_or_zero(yd + (size_t)t * M, ml, M);
                double at = cabs2(gs);
                cd num = cmulc(y, gs);              // conj(g_m) y_m
                cd q = cmul(ss, gs);
#pragma unroll
                for (int off = 1; off < 8; off <<= 1) {
                    at += shfl_xor_d(at, off);
                    num = cadd(num, shfl_xor_c(num, off));
                    q = cadd(q, shfl_xor_c(q, off));
                }
                const cd mu = cscale(num, 1.0 / (at + v2));
                const cd den = cmk(q.x + v2, q.y);
                cd c = cscale(cconj(den), v2 / cabs2(den));
                c.x += cabs2(mu);
                if (lane == 0) {
                    cm[2 * tt] = c;
                    cm[2 * tt + 1] = cconj(mu);
                }
            }
            __syncthreads();
            // W += c_t conj(psi_i) psi_j, rhs[n][m] += y_t[m] conj(mu_t) conj(psi_t[n])
            for (int tt = 0; tt < nc; ++tt) {
                const int t = c0 + tt;
                const cd* ps = psid + (size_t)t * N;
                const cd c = cm[2 * tt], mc = cm[2 * tt + 1];
                cd pj[R];
#pragma unroll
                for (int y = 0; y < R; ++y) pj[y] = ld_or_zero(ps, tj + 16 * y, N);
#pragma unroll
                for (int x = 0; x < R; ++x) {
                    const cd wi = cmulc(c, ld_or_zero(ps, ti + 16 * x, N));
#pragma unroll
                    for (int y = 0; y < R; ++y) acc[x][y] = cfma(acc[x][y], wi, pj[y]);
                }
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (en[k] >= 0)
                        rr[k] = cfmac(rr[k], cmul(yd[(size_t)t * M + em[k]], mc), ps[en[k]]);
            }
        }

        // ---- the augmented system into LDS (the last reads of W are behind a barrier)
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y)
                if (ti + 16 * x < N && tj + 16 * y < N) W[(ti + 16 * x) * LD + tj + 16 * y] = acc[x][y];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (en[k] >= 0) W[en[k] * LD + N + em[k]] = rr[k];
        __syncthreads();

        // ---- Gauss-Jordan with partial pivoting; every wave finds the pivot itself
        const double dmax2 = wave_max_dpp(lane < N ? cabs2(W[lane * LD + lane]) : 0.0);
        const double tol2 = 1e-28 * dmax2;          // (1e-14 max_i |A_ii|)^2
        unsigned long long used = 0;
        for (int k = 0; k < N; ++k) {
            double d = INFINITY;
            int idx = lane;
            if (lane < N && !((used >> lane) & 1ull)) d = -cabs2(W[lane * LD + k]);
            wave_argmin_dpp(d, idx);
            if (!(-d > tol2)) {                     // also NaN, and no candidate
                singular = true;
                break;
            }
            const int p = idx;
            used |= 1ull << p;
            if (tid == 0) piv[k] = p;
            if (gi < N && gi != p) {
                const cd pv = W[p * LD + k];
                const cd inv = cscale(cconj(pv), fast_rcp64(cabs2(pv)));
                const cd l = cmul(W[gi * LD + k], inv);
                for (int j = k + 1 + gc; j < N + M; j += tpr)
                    W[gi * LD + j] = csub(W[gi * LD + j], cmul(l, W[p * LD + j]));
            }
            __syncthreads();
        }
        if (singular) break;                        // G stays at the last finite iterate

        // ---- G_new[k][m] = conj(rhs[p_k][m] / W[p_k][k])
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (en[k] >= 0) {
                const int p = piv[en[k]];
                const cd pv = W[p * LD + en[k]];
                const cd z = cmul(W[p * LD + N + em[k]], cscale(cconj(pv), fast_rcp64(cabs2(pv))));
                const cd gn = cconj(z);
                Gs[en[k] * M + em[k]] = gn;
                g[(size_t)en[k] * M + em[k]] = gn;
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = ns + 8 * i;
            greg[i] = (ml < M && n < N) ? Gs[n * M + ml] : czero();
        }
    }
    if (tid == 0 && a.status) a.status[b] = a.status0 | (singular ? SBCE_STATUS_SINGULAR : 0);
}

size_t approx_lds_bytes(int N, int M) {
    return ((size_t)N * apx_ld(N, M) + (size_t)N * M + 2 * kApxChunk * 2) * sizeof(cd) +
           (size_t)N * sizeof(int);
}

template <int R>
hipError_t launch_r(const ApproxArgs& a, hipStream_t s) {
    const size_t lds = approx_lds_bytes(a.N, a.M);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)approx_em_kernel<R>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(approx_em_kernel<R>, dim3(a.B), dim3(kApxThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace

bool approx_supported(int N, int M) { return N >= 1 && N <= kApxMaxN && M >= 1 && M <= kApxMaxM; }

hipError_t launch_approx(const ApproxArgs& a, hipStream_t s) {
    switch ((a.N + 15) / 16) {
        case 1: return launch_r<1>(a, s);
        case 2: return launch_r<2>(a, s);
        case 3: return launch_r<3>(a, s);
        default: return launch_r<4>(a, s);
    }
}

}  // namespace sbce
