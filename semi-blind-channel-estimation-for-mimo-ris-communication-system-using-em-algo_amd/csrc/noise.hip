// The M-step's second half: the noise-variance update of sbce_noise_var / sbce_em_noise
// (include/sbce.h).  Per trial, from the theta the M-step just produced and the moments
// (m_t, S_t) the E-step of the same iteration left in the workspace,
//   Q       = sum_pilots ||y_p - H_c u_p||^2 + sum_data ( ||y_t - H_t m_t||^2 + tr(H_t C_t H_t^H) ),
//   sigma^2 = Q / (n_rx (T_p + T_d)),   C_t = S_t - m_t m_t^H,
//   H_t[r][a] = sum_p psi_t[p] theta[(p n_tx + a) n_rx + r]      (the effective channel),
// in the residual form: both data terms are non-negative up to rounding (the expanded form
// ||y||^2 - 2 Re(y^H H m) + tr(H S H^H) cancels at high SNR).  The data term separates over the
// receive antennas, sum_r ( |y_r - h_r m|^2 + h_r C h_r^H ) with h_r row r of H_t, so one work
// item is (symbol, antenna) and keeps n_tx complex accumulators.
//
// noise_partial_kernel   grid (nblk, B), 256 threads.  Items of a trial in one line: the data
//   items t n_rx + r, then the pilot items T_d n_rx + t n_rx + r; block k owns items
//   [256 k, 256 k + 256).  Consecutive lanes are the antennas of one symbol (r fastest), so the
//   theta reads of a p-step are contiguous in LDS and psi_t, m_t, S_t are one address per symbol
//   (broadcast).  theta and the block's psi rows are staged through LDS in tiles of kNoiseTP
//   phases (the whole theta does not fit at P = 257, n_tx = n_rx = 8); the psi rows are padded by
//   one element, which takes the 128-byte row stride off the ds_read_b128 bank pattern.  Pilot
//   items walk the same tiles with u_p read from global memory.
// Determinism: no atomics.  A block's sum is the fixed-order DPP wave reduction (wave_sum_dpp),
//   then the four wave sums added in wave order (block_sum4, shared with loglik.hip's pilot
//   items); block sums go to part[b][k]; nblk and the
//   item -> block map depend on (T_d, T_p, n_rx) only, never on B.
// noise_final_kernel     one thread per trial: part[b][0..nblk) in index order, the floor and
//   keep-previous rules, varn_est[b] and (optionally) varn_hist[b][it].
#include "sbce_internal.h"

namespace sbce {

namespace {

constexpr int kNoiseTP = 8;          // phases per LDS tile
constexpr int kNoiseThreads = 256;

// rows of the psi tile: the symbols 256 consecutive items can touch (<= 256 / NR + 2)
__host__ __device__ inline int noise_tile_rows(int NR, int Td) {
    const int n = kNoiseThreads / NR + 2;
    return n < Td ? n : Td;
}

template <int NT>
__global__ __launch_bounds__(kNoiseThreads) void noise_partial_kernel(NoiseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char noise_smem[];
    const int NR = a.NR, P = a.P, Td = a.Td, Tp = a.Tp;
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (a.done && a.done[b]) return;                 // block-uniform: the trial has stopped
    const int rows = noise_tile_rows(NR, Td);
    cd* th_s = (cd*)noise_smem;                      // [kNoiseTP][NT][NR]
    cd* ps_s = th_s + kNoiseTP * NT * NR;            // [rows][kNoiseTP + 1]
    double* red = (double*)(ps_s + rows * (kNoiseTP + 1));   // [4]

    const int nd = Td * NR, ni = nd + Tp * NR;
    const int i0 = blk * kNoiseThreads, i = i0 + tid;
    const bool is_d = i < nd, is_p = !is_d && i < ni;
    const int j = is_d ? i : (is_p ? i - nd : 0);
    const int t = j / NR, r = j - t * NR;
    // the block's data symbols [s0, s1)
    const int s0 = i0 / NR;
    const int ie = i0 + kNoiseThreads < nd ? i0 + kNoiseThreads : nd;
    const int s1 = (ie + NR - 1) / NR;
    const int ns = s1 > s0 ? s1 - s0 : 0;            // <= rows

    const cd* thg = a.theta + (size_t)b * P * NT * NR;
    const cd* psg = a.psid + ((size_t)b * Td + (ns ? s0 : 0)) * P;
    const cd* upg = a.up + ((size_t)b * Tp + (is_p ? t : 0)) * ((size_t)P * NT);
    cd h[NT];                                        // data: row r of H_t; pilots: h[0] = (H_c u)_r
#pragma unroll
    for (int ai = 0; ai < NT; ++ai) h[ai] = czero();
    for (int p0 = 0; p0 < P; p0 += kNoiseTP) {
        const int np = P - p0 < kNoiseTP ? P - p0 : kNoiseTP;
        __syncthreads();                             // the previous tile is consumed
        for (int e = tid; e < np * NT * NR; e += kNoiseThreads)
            th_s[e] = thg[(size_t)p0 * NT * NR + e];
        for (int e = tid; e < ns * kNoiseTP; e += kNoiseThreads) {
            const int s = e / kNoiseTP, pp = e - s * kNoiseTP;
            if (pp < np) ps_s[s * (kNoiseTP + 1) + pp] = psg[(size_t)s * P + p0 + pp];
        }
        __syncthreads();
        if (is_d) {
            const cd* pr = ps_s + (t - s0) * (kNoiseTP + 1);
            for (int pp = 0; pp < np; ++pp) {
                const cd ps = pr[pp];
#pragma unroll
                for (int ai = 0; ai < NT; ++ai)
                    h[ai] = cfma(h[ai], ps, th_s[(pp * NT + ai) * NR + r]);
            }
        } else if (is_p) {
            for (int pp = 0; pp < np; ++pp)
#pragma unroll
                for (int ai = 0; ai < NT; ++ai)
                    h[0] = cfma(h[0], th_s[(pp * NT + ai) * NR + r], upg[(p0 + pp) * NT + ai]);
        }
    }

    double q = 0.0;
    if (is_d) {
        const cd* mo = a.mom + ((size_t)b * Td + t) * (NT + NT * NT);
        cd e = a.yd[((size_t)b * Td + t) * NR + r];
#pragma unroll
        for (int ai = 0; ai < NT; ++ai) e = csub(e, cmul(h[ai], mo[ai]));
        q = cabs2(e);
        double tr = 0.0;                             // h C h^H, C = S - m m^H
#pragma unroll
        for (int ai = 0; ai < NT; ++ai) {
            cd w = czero();                          // sum_b C[a][b] conj(h[b])
#pragma unroll
            for (int bi = 0; bi < NT; ++bi)
                w = cfmac(w, csub(mo[NT + ai * NT + bi], cmulc(mo[ai], mo[bi])), h[bi]);
            tr += fma(h[ai].x, w.x, -h[ai].y * w.y);
        }
        q += tr;
    } else if (is_p) {
        q = cabs2(csub(a.yp[((size_t)b * Tp + t) * NR + r], h[0]));
    }
    q = block_sum4(wave_sum_dpp(q), red, tid & 63, tid >> 6);
    if (tid == 0) a.part[(size_t)b * a.nblk + blk] = q;
}

__global__ __launch_bounds__(256) void noise_final_kernel(NoiseFinalArgs f) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= f.B) return;
    double v = f.prev_t ? f.prev_t[b] : f.prev;      // the parameter before this update
    if (!(f.done && f.done[b])) {
        double q = 0.0;
        for (int k = 0; k < f.nblk; ++k) q += f.part[(size_t)b * f.nblk + k];
        const double s2 = q / f.denom;
        int flag = 0;
        if (!isfinite(q)) {
            flag = SBCE_STATUS_NOISE;                // the previous value is kept
        } else if (s2 < f.varn_min * f.varn_min) {
            v = f.varn_min;
            flag = SBCE_STATUS_NOISE;
        } else {
            v = sqrt(s2);
        }
        if (f.status) {
            if (f.status_base >= 0) f.status[b] = f.status_base | flag;
            else if (flag) f.status[b] |= flag;
        }
        f.varn_est[b] = v;
    }
    if (f.hist) f.hist[(size_t)b * f.iters + f.it] = v;
}

__global__ __launch_bounds__(256) void noise_init_kernel(int B, double* est, const double* varn_t,
                                                         double varn) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) est[b] = varn_t ? varn_t[b] : varn;
}

}  // namespace

int noise_nblk(const Problem& pb) {
    const long items = ((long)pb.Td + pb.Tp) * pb.NR;
    return (int)((items + kNoiseThreads - 1) / kNoiseThreads);
}

hipError_t launch_noise_init(int B, double* est, const double* varn_t, double varn, hipStream_t s) {
    hipLaunchKernelGGL(noise_init_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, est, varn_t,
                       varn);
    return hipGetLastError();
}

hipError_t launch_noise_partial(const Problem& pb, NoiseArgs a, hipStream_t s) {
    a.NR = pb.NR; a.P = pb.P; a.Tp = pb.Tp; a.Td = pb.Td;
    a.nblk = noise_nblk(pb);
    const size_t lds = ((size_t)kNoiseTP * pb.NT * pb.NR +
                        (size_t)noise_tile_rows(pb.NR, pb.Td) * (kNoiseTP + 1)) * sizeof(cd) +
                       4 * sizeof(double);
    const dim3 grid(a.nblk, pb.B), block(kNoiseThreads);
    switch (pb.NT) {
#define SBCE_NOISE(n) case n: hipLaunchKernelGGL(noise_partial_kernel<n>, grid, block, lds, s, a); break;
        SBCE_NOISE(1) SBCE_NOISE(2) SBCE_NOISE(3) SBCE_NOISE(4) SBCE_NOISE(5) SBCE_NOISE(6)
        SBCE_NOISE(7) SBCE_NOISE(8)
#undef SBCE_NOISE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_noise_final(const Problem& pb, NoiseFinalArgs f, hipStream_t s) {
    f.B = pb.B;
    f.nblk = noise_nblk(pb);
    f.denom = (double)pb.NR * ((double)pb.Tp + (double)pb.Td);
    hipLaunchKernelGGL(noise_final_kernel, dim3((pb.B + 255) / 256), dim3(256), 0, s, f);
    return hipGetLastError();
}

}  // namespace sbce
