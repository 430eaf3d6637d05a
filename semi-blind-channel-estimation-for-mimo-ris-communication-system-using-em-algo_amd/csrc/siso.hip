// Batched soft-in / soft-out decoder of a rate-1/n feed-forward binary code (include/sbce.h
// sbce_siso_decode): the exact BCJR forward-backward recursion in the log domain
// (log-MAP, or max-log-MAP with SBCE_DETECT_MAXLOG).
//
// Geometry.  One lane per trellis state, S = 2^(K-1) lanes per codeword, G = 64 / S codewords per
// wave (lane = g S + s); the remainder lanes of the last group of a call repeat the loads of the
// last codeword and store nothing but their workspace slots.  A workgroup is two waves over the
// SAME G codewords: wave F runs alpha forward from step 0, wave B runs beta backward from step T,
// each as far as the meeting point h = ceil(T / 2), storing one metric row per step (alpha_t into
// slot t for t < h, beta_{t+1} into slot t for t >= h: T rows of 64 doubles per workgroup in the
// global workspace).  After one barrier each wave walks on through the other half and forms the
// outputs of its steps from its running metric and the stored one: wave F those of t >= h, wave B
// those of t < h.  The dependent chain of a codeword is T steps long instead of 2 T.
//
// Trellis.  s' = (u << (K-2)) | (s >> 1): both branches into s' carry the input u = msb(s') and
// come from p0 = (2 s') mod S and p1 = p0 | 1; the successors of s are s >> 1 (u = 0) and
// (s >> 1) | S/2 (u = 1).  Neighbour metrics come by ds_bpermute; since every generator taps the
// current input, c_j(s, 1) = 1 - c_j(s, 0), so every lane puts exactly one of its two branches into
// each of the 2 (n + 1) classes of a step.
//
// Numerics.  -inf is an ordinary metric (lse2, class_lse below); every class sum is shifted by ITS
// OWN maximum, never by the step's: with the global shift a class 745 below the step's best branch
// -- contradictory or merely decisive inputs reach that at d_free 64 -- would underflow to an
// "empty" class.  Normalisation rule: the metric row of step t+1 is stored minus alpha_t(0)
// (beta_{t+2}(0) backward), state 0's metric of the row it was formed from; state 0 is reachable in
// both directions, so the constant is finite, it is known before the step's lse (off the chain),
// and |metrics| stay bounded by a few constraint lengths of |L|.  It cancels in every output.
// Every order of summation is fixed by (K, n, T, flags): reductions are butterflies inside the S
// lanes of a codeword, so codeword b's bits do not depend on its lane group or on the batch.
#include "ep_prior.h"
#include "sbce_internal.h"

namespace sbce {
namespace {

constexpr int kSisoThreads = 128;

__device__ __forceinline__ double siso_sanitise(double v) {
    v = v != v ? 0.0 : v;
    return fmin(fmax(v, -kPriorClamp), kPriorClamp);
}

// log(e^a + e^b), max-shifted; lse of two -inf is -inf
template <bool MAXLOG>
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    if constexpr (MAXLOG) return m;
    const double d = fmin(a, b) - m;          // <= 0, -inf, or NaN when both are -inf
    return m == -INFINITY ? m : m + log1p(fexp_neg(d));
}

// max / sum over the S lanes of a codeword (S-aligned lane groups): DPP inside a row of 16, then
// ds_bpermute butterflies.  Every lane of the group ends with the same bits.
template <int S, bool MAX>
__device__ __forceinline__ double group_red(double v) {
    auto op = [](double a, double b) { return MAX ? fmax(a, b) : a + b; };
    if constexpr (S >= 2) v = op(v, dpp_d<0xB1>(v));
    if constexpr (S >= 4) v = op(v, dpp_d<0x4E>(v));
    if constexpr (S >= 8) v = op(v, dpp_d<0x141>(v));
    if constexpr (S >= 16) v = op(v, dpp_d<0x140>(v));
    if constexpr (S >= 32) v = op(v, shfl_xor_d(v, 16));
    if constexpr (S >= 64) v = op(v, shfl_xor_d(v, 32));
    return v;
}

// lse over a codeword's lanes of x (one class member per lane), shifted by the class maximum
template <int S, bool MAXLOG>
__device__ __forceinline__ double class_lse(double x) {
    const double m = group_red<S, true>(x);
    if constexpr (MAXLOG) return m;
    const double e = m == -INFINITY ? 0.0 : fexp_neg(x - m);
    const double z = group_red<S, false>(e);
    return m == -INFINITY ? m : m + log(z);
}

// The L-values of one trellis step, sanitised
template <int N>
struct SisoStep {
    double l[N];
    double la;
    bool tail;        // no u = 1 branch
};

// gamma(s, u) = -sum_j c_j L_j - u La in this order; cm: bit j = c_j(s, u)
template <int N>
__device__ __forceinline__ double siso_gamma(const SisoStep<N>& st, int cm, int u) {
    double g = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) g -= (cm >> j) & 1 ? st.l[j] : 0.0;
    g -= u ? st.la : 0.0;
    return g;
}

// TWO = false (the A/B build's one-wave arm, sbce_debug_siso_onewave): a 64-thread workgroup runs
// alpha over all T steps and then beta with every output -- the same expressions on the same
// values, so the same bits -- for the A/B timing of the split.
template <int S, int N, bool MAXLOG, bool TWO>
__global__ __launch_bounds__(TWO ? kSisoThreads : 64) void siso_kernel(SisoArgs a) {
    constexpr int G = 64 / S;
    constexpr int kAll = (1 << N) - 1;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int s = lane & (S - 1);
    const int base = lane - s;
    const long long bq = (long long)blockIdx.x * G + lane / S;
    const bool live = bq < a.B;
    const size_t b = (size_t)(live ? bq : a.B - 1);
    const int T = a.T, K = a.K, ninfo = a.ninfo;
    const int nc = T * N;
    const int h = TWO ? (T + 1) >> 1 : T;
    const double* lc = a.lc + b * (size_t)nc;
    const double* la = a.la ? a.la + b * (size_t)ninfo : nullptr;
    double* ws = a.ws + (size_t)blockIdx.x * (size_t)T * 64;

    // the branch code bits of this lane
    auto code = [&](int st, int u) {
        const int w = (u << (K - 1)) | st;
        int cm = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) cm |= (__popc(w & a.g[j]) & 1) << j;
        return cm;
    };
    const int uin = s >> (K - 2);                    // the input of both branches INTO s
    const int p0 = (2 * s) & (S - 1), p1 = p0 | 1;   // their origins
    const int s0 = s >> 1, s1 = s0 | (S >> 1);       // the successors of s under u = 0, 1
    const int cin0 = code(p0, uin), cin1 = code(p1, uin);
    const int co0 = code(s, 0), co1 = co0 ^ kAll;
    const int ap0 = (base + p0) * 4, ap1 = (base + p1) * 4, as0 = (base + s0) * 4,
              as1 = (base + s1) * 4, az = base * 4;

    auto load = [&](int t) {
        SisoStep<N> st;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int k = t * N + j;
            st.l[j] = siso_sanitise(lc[a.perm ? a.perm[k] : k]);
        }
        st.tail = t >= ninfo;
        st.la = la && !st.tail ? siso_sanitise(la[t]) : 0.0;
        return st;
    };
    // alpha_{t+1} from alpha_t (this lane's state is the branch's END)
    auto fwd = [&](double al, const SisoStep<N>& st) {
        const double a0 = bperm_d(al, ap0) + siso_gamma<N>(st, cin0, uin);
        const double a1 = bperm_d(al, ap1) + siso_gamma<N>(st, cin1, uin);
        const double v = (st.tail && uin) ? -INFINITY : lse2<MAXLOG>(a0, a1);
        return v - bperm_d(al, az);
    };
    // beta_t from beta_{t+1} (this lane's state is the branch's START)
    auto bwd = [&](double be, const SisoStep<N>& st) {
        const double b0 = siso_gamma<N>(st, co0, 0) + bperm_d(be, as0);
        const double n1 = siso_gamma<N>(st, co1, 1) + bperm_d(be, as1);
        return lse2<MAXLOG>(b0, st.tail ? -INFINITY : n1) - bperm_d(be, az);
    };
    int nerr = 0;
    // the outputs of step t from alpha_t(s) and beta_{t+1} at the two successors of s
    auto emit = [&](int t, double al, double be0, double be1, const SisoStep<N>& st) {
        const double A0 = (al + siso_gamma<N>(st, co0, 0)) + be0;
        const double A1 = st.tail ? -INFINITY : (al + siso_gamma<N>(st, co1, 1)) + be1;
        if (t < ninfo && (a.lapp || a.uhat || a.err)) {
            const double L = class_lse<S, MAXLOG>(A0) - class_lse<S, MAXLOG>(A1);
            if (live && s == 0) {
                const int u = L < 0.0 ? 1 : 0;
                if (a.lapp) a.lapp[b * (size_t)ninfo + t] = L;
                if (a.uhat) a.uhat[b * (size_t)ninfo + t] = u;
                if (a.err) nerr += u != (a.utrue[b * (size_t)ninfo + t] != 0);
            }
        }
        if (a.lec) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const bool c0 = (co0 >> j) & 1;      // c_j(s, 0); c_j(s, 1) is its complement
                const double L = class_lse<S, MAXLOG>(c0 ? A1 : A0) -
                                 class_lse<S, MAXLOG>(c0 ? A0 : A1);
                if (live && s == 0) {
                    const int k = t * N + j;
                    a.lec[b * (size_t)nc + (a.perm ? a.perm[k] : k)] = L - st.l[j];
                }
            }
        }
    };

    double m;      // the running metric: alpha (wave 0) or beta (wave 1)
    if (wave == 0) {
        m = s == 0 ? 0.0 : -INFINITY;
        for (int t = 0; t < h; ++t) {
            ws[(size_t)t * 64 + lane] = m;
            m = fwd(m, load(t));
        }
    }
    if (wave == 1 || !TWO) {
        m = (a.term && s != 0) ? -INFINITY : 0.0;
        for (int t = T - 1; t >= h; --t) {
            ws[(size_t)t * 64 + lane] = m;
            m = bwd(m, load(t));
        }
    }
    __syncthreads();
    if (wave == 0 && TWO) {
        for (int t = h; t < T; ++t) {
            const SisoStep<N> st = load(t);
            const double* row = ws + (size_t)t * 64 + base;
            emit(t, m, row[s0], row[s1], st);
            m = fwd(m, st);
        }
    } else {
        for (int t = h - 1; t >= 0; --t) {
            const SisoStep<N> st = load(t);
            const double al = ws[(size_t)t * 64 + lane];
            emit(t, al, bperm_d(m, as0), bperm_d(m, as1), st);
            m = bwd(m, st);
        }
    }
    if (a.err && live && s == 0 && nerr) atomicAdd(a.err + b, nerr);
}

// err[b] = 0 ahead of the decoder's integer adds (a kernel, as linear_zero_kernel: a captured
// graph then holds kernel nodes only)
__global__ __launch_bounds__(256) void siso_zero_kernel(int32_t* err, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) err[i] = 0;
}

#if SBCE_AB
bool g_siso_onewave = false;
#endif

template <int S, int N>
hipError_t siso_launch(const SisoArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)siso_groups(a.B, a.K)), block(kSisoThreads);
#if SBCE_AB
    if (g_siso_onewave) {
        if (a.maxlog)
            hipLaunchKernelGGL((siso_kernel<S, N, true, false>), grid, dim3(64), 0, s, a);
        else
            hipLaunchKernelGGL((siso_kernel<S, N, false, false>), grid, dim3(64), 0, s, a);
        return hipGetLastError();
    }
#endif
    if (a.maxlog)
        hipLaunchKernelGGL((siso_kernel<S, N, true, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((siso_kernel<S, N, false, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

template <int S>
hipError_t siso_launch_n(const SisoArgs& a, hipStream_t s) {
    return a.N == 2 ? siso_launch<S, 2>(a, s) : siso_launch<S, 3>(a, s);
}

}  // namespace

void siso_debug_onewave(int on) {
#if SBCE_AB
    g_siso_onewave = on != 0;
#else
    (void)on;
#endif
}

bool siso_supported(int K, int N) { return K >= 3 && K <= 7 && (N == 2 || N == 3); }

long long siso_groups(int B, int K) {
    const int G = 64 >> (K - 1);
    return ((long long)B + G - 1) / G;
}

size_t siso_ws_bytes(int B, int K, int T) {
    return (size_t)siso_groups(B, K) * (size_t)T * 64 * sizeof(double);
}

hipError_t launch_siso(const SisoArgs& a, hipStream_t s) {
    if (!siso_supported(a.K, a.N) || a.T < 1 || a.T > kSisoMaxSteps) return hipErrorInvalidValue;
    if (a.err) {
        hipLaunchKernelGGL(siso_zero_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, s,
                           a.err, a.B);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    switch (a.K) {
        case 3: return siso_launch_n<4>(a, s);
        case 4: return siso_launch_n<8>(a, s);
        case 5: return siso_launch_n<16>(a, s);
        case 6: return siso_launch_n<32>(a, s);
        default: return siso_launch_n<64>(a, s);
    }
}

}  // namespace sbce
