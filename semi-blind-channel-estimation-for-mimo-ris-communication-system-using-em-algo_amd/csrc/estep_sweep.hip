// MFMA sweep of the exact E-step (the posterior and its reduced form: estep_valu.hip): the kernel,
// its geometry and dispatch, and the geometry the passes in front of it share (SweepPlan).
#include "sbce_internal.h"

namespace sbce {

namespace {

// ============================================================================
// MFMA variant (gfx950 FP64 matrix cores) for JA >= 16 and JB >= 16.
//
// One wave per symbol.  The hypothesis grid (i over A, k over B) is tiled in
// 16 x 16 tiles; each tile's distances
//     d_ik = (alpha_i + gamma_k) + sum_kk P'[i][kk] Q[kk][k],
// with P' = (-2 Re p_i, -2 Im p_i) and Q = (Re q_k, Im q_k) (K = 2*NR padded to
// a multiple of 4), come out of KPAD/4 chained v_mfma_f64_16x16x4f64 whose
// accumulator is initialised with alpha_i + gamma_k.  Lane l owns column
// k = 16*kt + (l & 15) and rows i = 16*t + (l >> 4) + 4*j (j < 4), so the
// per-k posterior sums (c_k, mu_k) are per lane, exactly like the VALU kernel.
// The VALU only does the running minimum, the skip test and (rarely, at high
// SNR) the exp/accumulate work, in parallel with the matrix pipe.
// The A operand is assembled per tile from two small LDS tables, -2 p_i =
// U_{s0} + V_{s1} (U_s = -2(y - h_0 x_s), V_s = 2 h_1 x_s, layout [kk][s]:
// conflict-free ds_read_b64), and alpha_i = ||p_i||^2 is tabulated 256 at a time.
// ============================================================================

// Initial bound for the hypothesis sweep: the distance ||y - H x_c||^2 of x_c = the
// per-stream nearest constellation points of the regularised LS estimate
// (H^H H + reg I)^-1 H^H y.  x_c is a real hypothesis, so its weight bounds the posterior
// maximum from below: as the initial log-sum-exp shift it loses nothing, and as the initial
// hard-decision bound (plus a rounding margin) it keeps the argmin.  At medium and high SNR
// x_c is the ML point, the running minimum never moves and nearly every tile group is
// dismissed by one comparison.  Wave-uniform (every lane computes the same value); `scale`
// bounds the magnitude of the terms a tile distance is assembled from (rounding margin).
template <int NT, int NR>
__device__ double candidate_distance(const cd* H, const cd* yg, const cd* s_cons, int M,
                                     double reg, cd* scratch, int lane, double& scale) {
    cd* sG = scratch;            // [NT][NT]
    cd* sHy = scratch + 16;      // [NT]
    if (lane < NT * NT) {
        const int u = lane / NT, v = lane - u * NT;
        cd acc = czero();
#pragma unroll
        for (int r = 0; r < NR; ++r) acc = cfmac(acc, H[v * NR + r], H[u * NR + r]);
        if (u == v) acc.x += reg;
        sG[lane] = acc;
    } else if (lane >= 32 && lane < 32 + NT) {
        const int u = lane - 32;
        cd acc = czero();
#pragma unroll
        for (int r = 0; r < NR; ++r) acc = cfmac(acc, yg[r], H[u * NR + r]);
        sHy[u] = acc;
    }
    wave_sync();
    // complex Cholesky G = L L^H and the two triangular solves, in registers
    cd Lm[NT][NT];
    double dinv[NT];
    cd z[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        double d = sG[j * NT + j].x;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= cabs2(Lm[j][k]);
        const double inv = fast_rsqrt(fmax(d, 1e-300));
        dinv[j] = inv;
#pragma unroll
        for (int i = j + 1; i < NT; ++i) {
            cd s = sG[i * NT + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = csub(s, cmulc(Lm[i][k], Lm[j][k]));
            Lm[i][j] = cscale(s, inv);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        cd s = sHy[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = csub(s, cmul(Lm[i][k], z[k]));
        z[i] = cscale(s, dinv[i]);
    }
#pragma unroll
    for (int i = NT - 1; i >= 0; --i) {
        cd s = z[i];
#pragma unroll
        for (int k = i + 1; k < NT; ++k) s = csub(s, cmul(cconj(Lm[k][i]), z[k]));
        z[i] = cscale(s, dinv[i]);
    }
    // nearest constellation point per stream: lanes 16 q .. 16 q + 15 handle stream q
    const int qa = lane >> 4;
    cd za = z[0];
#pragma unroll
    for (int q = 1; q < NT; ++q) za = csel(qa == q, z[q], za);
    double bd = INFINITY;
    int bs = 0;
    if (qa < NT)
        for (int s = lane & 15; s < M; s += 16) {
            const double dd = cabs2(csub(za, s_cons[s]));
            if (dd < bd) { bd = dd; bs = s; }
        }
    for (int off = 8; off >= 1; off >>= 1) {
        const double od = shfl_xor_d(bd, off);
        const int os = __shfl_xor(bs, off);
        if (od < bd || (od == bd && os < bs)) { bd = od; bs = os; }
    }
    cd x[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) x[q] = s_cons[__shfl(bs, 16 * q)];
    double d0 = 0.0, sc = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        cd res = yg[r];
        sc += cabs2(res);
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const cd hx = cmul(H[q * NR + r], x[q]);
            res = csub(res, hx);
            sc += NT * cabs2(hx);
        }
        d0 += cabs2(res);
    }
    wave_sync();                 // scratch is reused by the caller
    scale = sc;
    return d0;
}


constexpr int kMfmaWaves = 2;
constexpr int kChunk = 256;
constexpr int kScreenD = 256;   // per-wave LDS doubles of the V16 FP32 screen tables

typedef float f4v __attribute__((ext_vector_type(4)));

// Per-wave LDS doubles of the MFMA sweep: heff | alpha | U | V | Q2 | lb | scratch (128) |
// 2 x staged record (DMA double buffer: 128 + 32 done words, or the record itself) |
// FP32 screen tables (V16: alpha and U as floats, kScreenD doubles)
constexpr int mfma_rec_d(int rec_words) { return 2 * (rec_words <= 128 ? 160 : (rec_words + 1) / 2 * 2 + 32); }
// one half of that double buffer in the V16 layout (record 4 + 2 NT NR + 16 + 6 NR, y_t 2 NR)
constexpr int mfma_rec_half_v16(int NT, int NR) { return mfma_rec_d(4 + 2 * NT * NR + 16 + 8 * NR) / 2; }
// ... | per-group bound tables (V16, i.e. M = 16 with a 256-row chunk: U', V', Q' as floats,
// 64 steps each, then 256 floats that hold the projected vectors and after them alpha')
constexpr int mfma_tri_d(int steps) { return 3 * 64 * steps / 2 + 128; }
constexpr int mfma_tab_d(int NO, int chunk, int steps, int M, int nkt_pad, int rec_words) {
    return (2 * NO + chunk + 3 * (4 * steps) * M + nkt_pad + 128 + 1) / 2 * 2 + mfma_rec_d(rec_words) +
           kScreenD + (M == 16 && chunk == 256 ? mfma_tri_d(steps) : 0);
}
constexpr int kTriGate = 4;     // tile groups of a symbol at the screen before its bound tables are built

struct MfmaConst {
    int B, Td, P, M, lm;
    int JA, JB, chunk, nparts;
    int tab_d;                 // per-wave LDS doubles
    double inv_s2, thr_d;
    double reg;                // ridge of the candidate's LS estimate (0.1 varn^2)
    int nkt_pad;               // column tiles JB / 16, rounded up to even (LDS carve)
    int prune;                 // column-tile bounds on (SBCE_ESTEP_PRUNE=0 disables: A/B runs)
    int count;                 // diagnostic MFMA count (SBCE_ESTEP_COUNT=1)
    int prep_stride;           // doubles per symbol of EstepArgs::prep
    int rowb_off;              // offset of the row-tile bound vectors in a prep record
    int rowb;                  // row-tile bounds on (NT = 4 with a prep record)
    int rec_words;             // prep record + y_t, doubles (staged per symbol in LDS)
    int spw;                   // symbols per wave (consecutive; the next record prefetched)
    int screen;                // V16 FP32 screen of the tile groups (SBCE_ESTEP_F32=0 disables)
    int tri;                   // V16 per-group bounds T_3 / T_1 (SBCE_ESTEP_TRI: 0 off, 1 built once
                               // kTriGate groups of the symbol reached the screen, 2 always built)
    int twopass;               // V16 soft sweep: search, then accumulate (A/B build: SBCE_ESTEP_TWOPASS=0
                               // is the one-pass sweep; the product build has the two-pass one alone)
    int order;                 // V16 soft sweep: best-first column tiles and row blocks (A/B build:
                               // SBCE_ESTEP_ORDER=0 is the natural order; the product build has it on)
};

// V16 (M == 16, NA == 2): the A operand's V term, V[kk][i & 15] = V[kk][lane & 15], is the
// same for every tile, so it is hoisted into registers (one LDS read + add per MFMA
// instead of two reads + add).  gamma_k is not added to the 16 accumulators: the skip
// tests use min(acc) + gamma and the rare exp path adds it back.  (PMC at cfg1 showed
// the f64 VALU work between the MFMAs, which does not co-execute with them, as the
// limiter: 40 % MFMA busy.)
// Exact lower bounds per column tile (16 consecutive k): every hypothesis (i, k) has
//   d_ik = ||y - H_A x_A(i) - H_B x_B(k)||^2 >= min_x ||(y - H_B x_B(k)) - H_A x||^2
//        = ||P (y - H_B x_B(k))||^2,      P = projector onto span(H_A)^perp
// (the best continuous x_A can do no better: the partial distance of a sphere decoder).
// A tile whose bound exceeds the skip bound holds only hypotheses whose weights are below
// e^-50 of the posterior maximum (soft) or that cannot be the argmin (hard), exactly the
// hypotheses the per-group test already discards, so the sweep skips their MFMAs.  P comes
// from a twice-orthogonalised Gram-Schmidt basis of H_A, lane r of each 8-lane group owning
// component r; a near-dependent H_A (or n_rx <= |A|, where P = 0) leaves the bounds at 0.
// Returns the magnitude scale of the bound terms (rounding margin).
template <int NT, int NR>
__device__ double column_tile_bounds(const cd* H, const cd* yg, const cd* s_cons, int M, int lm,
                                     int nkt, double* s_lb, cd* scratch, int lane) {
    constexpr int NA = NT / 2, NB = NT - NA;
    const int mask = M - 1;
    const int r = lane & 7;
    const bool own = r < NR;
    int xa[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) xa[i] = (lane ^ (32 >> i)) << 2;     // xor 32 .. 1
    auto rsum = [&](double v) {                                      // sum over the 8-lane group
#pragma unroll
        for (int i = 3; i < 6; ++i) v += bperm_d(v, xa[i]);
        return v;
    };
    auto rdot = [&](cd u, cd v) { return cmk(rsum(fma(v.x, u.x, v.y * u.y)),    // u^H v
                                             rsum(fma(v.y, u.x, -v.x * u.y))); };
    cd u[NA];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        cd v = own ? H[q * NR + r] : czero();
        const double h2 = rsum(cabs2(v));
#pragma unroll
        for (int rep = 0; rep < 2; ++rep)
#pragma unroll
            for (int j = 0; j < q; ++j) v = csub(v, cmul(u[j], rdot(u[j], v)));
        const double n2 = rsum(cabs2(v));
        ok = ok && h2 > 0.0 && n2 > 1e-6 * h2;
        u[q] = cscale(v, ok ? fast_rsqrt(n2) : 0.0);
    }
    cd w = own ? yg[r] : czero();
    double sc = rsum(cabs2(w));
    cd g[NB];
    double g2 = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        g[b] = own ? H[(NA + b) * NR + r] : czero();
        g2 += cabs2(g[b]);
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        w = csub(w, cmul(u[j], rdot(u[j], w)));
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = csub(g[b], cmul(u[j], rdot(u[j], g[b])));
    }
    if (lane < NR) {
        scratch[r] = w;
#pragma unroll
        for (int b = 0; b < NB; ++b) scratch[8 * (b + 1) + r] = g[b];
    }
    // scale: ||y||^2 + NB sum_b ||h_b||^2 max|c|^2 bounds every term of a bound
    double cmax2 = lane < M ? cabs2(s_cons[lane]) : 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) cmax2 = fmax(cmax2, bperm_d(cmax2, xa[i]));
    sc += NB * cmax2 * rsum(g2);
    wave_sync();
    for (int kt0 = 0; kt0 < nkt; kt0 += 4) {
        const int kt = kt0 + (lane >> 4);
        const int k = kt * 16 + (lane & 15);
        cd xb[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) xb[b] = s_cons[(k >> (lm * (NB - 1 - b))) & mask];
        double lb = 0.0;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            cd res = scratch[rr];
#pragma unroll
            for (int b = 0; b < NB; ++b) res = csub(res, cmul(scratch[8 * (b + 1) + rr], xb[b]));
            lb += cabs2(res);
        }
        if (!ok) lb = 0.0;
#pragma unroll
        for (int i = 2; i < 6; ++i) lb = fmin(lb, bperm_d(lb, xa[i]));   // 16-lane minimum
        if ((lane & 15) == 0 && kt < nkt) s_lb[kt] = lb;
    }
    wave_sync();
    return sc;
}

// Diagnostic (MfmaConst::count, SBCE_ESTEP_COUNT=1): FP64 MFMAs the sweep issued, for the
// executed-work roofline next to the bounds' pruning.
__device__ unsigned long long g_estep_mfma;
// ... and the V16 tile groups that survived every bound and reached the FP32 screen (the FP64
// test with the screen off): what the bounds leave the screen to reject.
__device__ unsigned long long g_estep_groups;
// ... and the tile groups the two-pass sweep's second pass recomputed (8 more FP64 MFMAs each,
// not in g_estep_mfma, which stays the search's count).
__device__ unsigned long long g_estep_pass2;

template <int NT, int NR, int MODE, int TU, bool V16, bool TP = false, bool REC = false>
__device__ __forceinline__ void estep_mfma_body(const EstepArgs& a, const MfmaConst& c) {
    static_assert(!V16 || NT == 4, "the V16 body is the n_tx = 4, M = 16 sweep");
    // TP: the two-pass soft sweep (search, then accumulate; see the second pass below)
    static_assert(!TP || (V16 && MODE == SBCE_ESTEP_SOFT && TU == 4), "two-pass: the V16 soft sweep");
    // V16 (n_tx = 4, M = 16): the layout constants are compile-time (LDS offsets fold into
    // immediates, one SGPR wave base); otherwise they come from MfmaConst
    const int k_M = V16 ? 16 : c.M;
    const int k_lm = V16 ? 4 : c.lm;
    const int k_JA = V16 ? 256 : c.JA;
    const int k_JB = V16 ? 256 : c.JB;
    const int k_chunk = V16 ? 256 : c.chunk;
    const int k_nkt_pad = V16 ? 16 : c.nkt_pad;
    const int k_rowb_off = V16 ? 4 + 2 * NT * NR + 16 : c.rowb_off;
    const int k_prep_stride = V16 ? k_rowb_off + 6 * NR : c.prep_stride;
    const int k_rec_words = V16 ? k_prep_stride + 2 * NR : c.rec_words;
    // TP: the second half of the record double buffer lies behind both waves' tables, and only
    // in a launch without a work list (a listed grab holds one symbol and prefetches none)
    constexpr int REC_H = mfma_rec_half_v16(NT, NR);
    const int k_tab_d = V16 ? mfma_tab_d(NT * NR, 256, (2 * NR + 3) / 4, 16, 16, k_rec_words) - (TP ? REC_H : 0)
                            : c.tab_d;
    constexpr int NA = NT / 2;
    constexpr int NB = NT - NA;
    constexpr int NO = NT * NR;
    constexpr int K2 = 2 * NR;
    constexpr int STEPS = (K2 + 3) / 4;
    constexpr int NPA = NA * (NA - 1) / 2;
    constexpr int NPB = NB * (NB - 1) / 2;
    static_assert(NA >= 1 && NA <= 2 && NB <= 2, "mfma E-step: 2 <= n_tx <= 4");

    // listed sweep: a block whose first wave has no list entry has no work at all (an empty
    // list is common: the launch then costs only its dispatch)
    if (a.list && (long)blockIdx.x * kMfmaWaves >= (long)a.list[(long)c.B * c.Td]) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cd* s_cons = reinterpret_cast<cd*>(smem);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: SGPR addresses
    const int lane = threadIdx.x & 63;
    double* wbase = reinterpret_cast<double*>(s_cons + 64) + (size_t)wave * k_tab_d;
    cd* s_heff = reinterpret_cast<cd*>(wbase);                 // NO
    double* s_al = wbase + 2 * NO;                             // chunk
    double* s_U = s_al + k_chunk;                              // [KPAD][M]
    double* s_V = s_U + 4 * STEPS * k_M;                       // [KPAD][M]   (NA == 2)
    double* s_Q2 = s_V + 4 * STEPS * k_M;                      // [KPAD][M]   (V16)
    double* s_lb = s_Q2 + 4 * STEPS * k_M;                     // [nkt] column-tile bounds
    double* s_tab = s_lb + k_nkt_pad;                          // scratch: 64 cd
    double* s_recb = s_tab + 128;                  // 2 x [prep record | y_t (128) | done (32)]
    // V16 FP32 screen: alpha (row order: the f32 MFMA's C/D row of value q is 4 (lane >> 4) + q,
    // not the f64 form's (lane >> 4) + 4 q) and U (s_U's layout) as floats
    float* s_al32 = reinterpret_cast<float*>(s_recb + (TP ? REC_H : mfma_rec_d(k_rec_words)));
    [[maybe_unused]] double* s_rec2 =
        reinterpret_cast<double*>(s_cons + 64) + (size_t)kMfmaWaves * k_tab_d + (size_t)wave * REC_H;
    auto rec_half = [&](int h) -> double* {
        if constexpr (TP) return h ? s_rec2 : s_recb;
        else return s_recb + h * 160;
    };
    float* s_U32 = s_al32 + 256;

    for (int i = threadIdx.x; i < k_M; i += blockDim.x) s_cons[i] = a.cons[i];
    __syncthreads();

    const long nsym = (long)c.B * c.Td;
    // With a work list (the prep pass's sphere enumeration resolved the other symbols) the
    // waves grab chunks of spw list entries from a counter until the list is exhausted;
    // otherwise each wave takes chunk (block, wave) of all symbols.
    const bool listed = a.list != nullptr;
    int32_t* cnt = listed ? a.list + nsym : nullptr;
    const long nwork = listed ? (long)__builtin_amdgcn_readfirstlane(cnt[0]) : nsym;
    // REC: a launch with a prep record, known at compile time (the in-kernel preparation of the
    // other launches, candidate_distance and column_tile_bounds, is what needs the most registers)
    const bool prep = REC || a.prep != nullptr;
    auto sym_of = [&](long gi) -> long { return listed ? (long)a.list[gi] : gi; };
    // listed: a wave's first entry is its global wave index (no atomic -- with a short or empty
    // list most waves exit at once; 4096 same-address atomics of an empty list cost ~50 us),
    // the later ones come from the counter, which starts past the first round
    bool first = true;
    for (;;) {
    long chunk_id;
    if (listed) {
        if (first) {
            chunk_id = (long)blockIdx.x * kMfmaWaves + wave;
        } else {
            int v = 0;
            if (lane == 0) v = atomicAdd(cnt + 1, 1);
            chunk_id = (long)gridDim.x * kMfmaWaves + __builtin_amdgcn_readfirstlane(__shfl(v, 0));
        }
        first = false;
    } else {
        chunk_id = (long)blockIdx.x * kMfmaWaves + wave;
    }
    // listed symbols are the expensive ones: one per grab (a chunk's symbols run in series)
    const int spw = listed ? 1 : c.spw;
    const long g0 = chunk_id * spw;
    if (g0 >= nwork) return;
    const long g1 = g0 + spw < nwork ? g0 + spw : nwork;
    // The wave's symbols g0 .. g1-1 in turn.  With a prep record, the next symbol's record,
    // y_t and done flag travel by LDS-DMA (global_load_lds: no VGPRs) into the other half of
    // a double buffer while the current symbol is swept; the sweep reads no global memory,
    // so the wait at the next symbol finds them landed.
    const bool dma = prep && k_rec_words <= 128;
    auto issue = [&](long g, double* dst) {
        int l = lane;                                           // recomputed per issue, not held
        asm volatile("" : "+v"(l));
        const int hs = k_prep_stride >> 1;                      // 16-byte words of the record
        const double* src = a.prep + (size_t)g * k_prep_stride;
        if (l < hs) src += 2 * l;
        else if (l < (k_rec_words >> 1))
            src = reinterpret_cast<const double*>(a.yd) + (size_t)g * 2 * NR + 2 * (l - hs);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        if (a.done)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(a.done + g / c.Td),
                (__attribute__((address_space(3))) void*)(dst + 128), 4, 0, 0);
    };
    if (dma) issue(sym_of(g0), s_recb);
    for (long gi = g0; gi < g1; ++gi) {
    const long gsym = sym_of(gi);
    const int cur = (int)((gi - g0) & 1);
    double* s_rec = rec_half(cur);
    int dn;
    if (dma) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this symbol's record has landed
        wave_sync();
        dn = a.done ? reinterpret_cast<const int*>(s_rec + 128)[0] : 0;
        if (gi + 1 < g1) issue(sym_of(gi + 1), rec_half(cur ^ 1));
    } else {
        dn = a.done ? a.done[gsym / c.Td] : 0;
        if (prep && !dn) {
            wave_sync();
            for (int e = lane; e < k_rec_words; e += 64)
                s_rec[e] = e < k_prep_stride
                    ? a.prep[(size_t)gsym * k_prep_stride + e]
                    : reinterpret_cast<const double*>(a.yd)[(size_t)gsym * 2 * NR + e - k_prep_stride];
            wave_sync();
        }
    }
    if (dn) continue;
    // lane index opaque per symbol: values derived from it (constellation points, LDS
    // addresses) are recomputed per symbol instead of being hoisted and held across the loop
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    [&, lane = lane_s]() {
    const int b = (int)(gsym / c.Td);
    const int t = (int)(gsym - (long)b * c.Td);
    const int mask = k_M - 1;
    // the trial's noise constants (per-trial variances, ABI 6): wave-uniform, kept in SGPRs
    double thr_d = c.thr_d, inv_s2 = c.inv_s2, reg = c.reg;
    if (a.varn_t) {
        const TrialNoise tn = trial_noise(a.varn_t[b]);
        thr_d = uniform_d(tn.thr_d);
        inv_s2 = uniform_d(tn.inv_s2);
        reg = uniform_d(tn.reg);
    }

    // ---------------- H_eff(t) ----------------
    if (prep) {
        // H_eff, bounds and y_t are read from the staged record (s_rec)
    } else {
        const cd* th = a.theta + (size_t)b * c.P * NO;
        const cd* ps = a.psid + (size_t)gsym * c.P;
        const int ntask = NO * c.nparts;
        cd* part = reinterpret_cast<cd*>(s_tab);
        if (lane < ntask) {
            const int o = lane % NO, pp = lane / NO;
            cd acc = czero();
            for (int p = pp; p < c.P; p += c.nparts) acc = cfma(acc, ps[p], th[p * NO + o]);
            part[lane] = acc;
        }
        wave_sync();
        if (lane < NO) {
            cd s2 = part[lane];
            for (int pp = 1; pp < c.nparts; ++pp) s2 = cadd(s2, part[pp * NO + lane]);
            s_heff[lane] = s2;
        }
        wave_sync();
    }
    const cd* H = prep ? reinterpret_cast<const cd*>(s_rec + 4) : s_heff;
    const double* lbp = prep ? s_rec + 4 + 2 * NO : s_lb;        // column-tile bounds
    double cscale_d, d0, lb_scale;
    if (prep) {                      // estep_prep_kernel did these per symbol
        d0 = s_rec[0];
        cscale_d = s_rec[1];
        lb_scale = s_rec[2];
    } else {
        d0 = candidate_distance<NT, NR>(H, a.yd + (size_t)gsym * NR, s_cons, k_M, reg,
                                        reinterpret_cast<cd*>(s_tab), lane, cscale_d);
        lb_scale = column_tile_bounds<NT, NR>(H, a.yd + (size_t)gsym * NR, s_cons, k_M, k_lm,
                                              k_JB >> 4, s_lb, reinterpret_cast<cd*>(s_tab), lane);
    }
    const double lb_margin = c.prune ? 1e-9 * lb_scale : INFINITY;
    // row-tile bounds (NT = 4): lane s0 < 16 of a surviving column tile kt evaluates
    // ||Py - x_s0 Ph_0 - x_kt Ph_2||^2, a lower bound of every hypothesis with first streams
    // (s0, kt); tile groups whose four bounds all exceed the skip bound are not swept
    const bool rowb = NT == 4 && V16 && prep && c.rowb;
    // row-tile bound tables (scratch s_tab[63..111], free on the prep path): per column tile kt (= x_2 index)
    //   n_kt = ||v_kt||^2 and a_kt = (P h_0)^H v_kt, v_kt = P y - x_kt P h_2, and ||P h_0||^2,
    // so the bound of row tile s0 is n_kt - 2 Re(conj(x_s0) a_kt) + |x_s0|^2 ||P h_0||^2
    double* s_rk = s_tab + 64;       // [16][3]
    if (rowb) {
        const double* rbp = s_rec + k_rowb_off;     // [3][NR] complex: P y, P h_0, P h_2
        double n = 0.0, nb0 = 0.0;
        cd av = czero();
        if (lane < 16) {
            const cd x2 = s_cons[lane];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const cd py = cmk(rbp[2 * r], rbp[2 * r + 1]);
                const cd p0 = cmk(rbp[2 * (NR + r)], rbp[2 * (NR + r) + 1]);
                const cd p2 = cmk(rbp[2 * (2 * NR + r)], rbp[2 * (2 * NR + r) + 1]);
                const cd v = csub(py, cmul(p2, x2));
                n += cabs2(v);
                nb0 += cabs2(p0);
                av = cfmac(av, v, p0);                 // p0^H v
            }
        }
        if (lane < 16) {
            s_rk[3 * lane] = n;
            s_rk[3 * lane + 1] = av.x;
            s_rk[3 * lane + 2] = av.y;
        }
        if (lane == 0) s_tab[63] = nb0;
        wave_sync();
    }

    // lane-level accumulators (see VALU kernel)
    // the running shift starts at a real hypothesis' distance (candidate_distance) plus a rounding
    // margin: the sweep's own distances (alpha + gamma - 2 Re p^H q) differ from d0 by rounding of
    // order eps * cscale_d, and a shift below every swept distance by more than 50 varn^2 would
    // skip every group and leave the posterior empty (0/0).  (A theta_0 ~1e13 from a near-singular
    // pinv puts that rounding at ~1e12 >> varn^2.)  The shift then falls to the true minimum.
    double mshift = d0 + 1e-10 * cscale_d;
    double tot_c = 0.0;
    cd tot_muA[NA];
    double nu[NA];
    cd kap = czero();
    cd tot_mB[NB];
    double tot_nB[NB];
    cd tot_kB = czero();
    cd tot_X[NA][NB];
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        tot_muA[q] = czero(); nu[q] = 0.0;
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) tot_X[q][bb] = czero();
    }
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) { tot_mB[bb] = czero(); tot_nB[bb] = 0.0; }
    double best_d = d0 + 1e-10 * cscale_d + 1e-300;   // admits the argmin (rounding margin)
                                                       // (== hard_bound below)
    int best_j = 0x7fffffff;

    // U_s = -2 (y - h_0 x_s),  V_s = 2 h_1 x_s  so that  -2 p_i = U_{s0(i)} + V_{s1(i)}
    // (NA == 1: -2 p_i = U_{i}).  Layout [kk][s]: conflict-free per-lane reads.
    {
        wave_sync();
        for (int e = lane; e < k_M * 4 * STEPS; e += 64) {
            const int kk = e >> k_lm, sx = e & mask;
            double u = 0.0, v = 0.0, q2 = 0.0;
            if (kk < K2) {
                const int r = kk >> 1;
                const cd x = s_cons[sx];
                const cd yv = prep ? reinterpret_cast<const cd*>(s_rec + k_prep_stride)[r]
                                   : a.yd[(size_t)gsym * NR + r];
                const cd pu = csub(yv, cmul(H[0 * NR + r], x));
                u = -2.0 * ((kk & 1) ? pu.y : pu.x);
                if (NA == 2) {
                    const cd hv = cmul(H[1 * NR + r], x);
                    v = 2.0 * ((kk & 1) ? hv.y : hv.x);
                }
                if (V16) {
                    const cd hq = cmul(H[NA * NR + r], x);
                    q2 = (kk & 1) ? hq.y : hq.x;
                }
            }
            s_U[e] = u;
            if (NA == 2) s_V[e] = v;
            if (V16) {
                s_Q2[e] = q2;
                s_U32[e] = (float)u;
            }
        }
        wave_sync();
    }
    const int col = lane & 15;
    const int rq = lane >> 4;
    // V16: hoisted A-operand V term, and the B operand q_k = h_NA x_kt + h_NA+1 x_col split
    // into a per-kt LDS row (s_Q2) plus a lane constant (q3reg)
    double vreg[STEPS], q3reg[STEPS];
    float vreg32[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int kk = 4 * s + rq;
        vreg[s] = V16 ? s_V[kk * 16 + col] : 0.0;
        vreg32[s] = (float)vreg[s];
        double q3 = 0.0;
        if (V16 && kk < K2) {
            const cd hx = cmul(H[(NA + 1) * NR + (kk >> 1)], s_cons[col]);
            q3 = (kk & 1) ? hx.y : hx.x;
        }
        q3reg[s] = q3;
    }
    const int xaddr16 = (lane ^ 16) << 2, xaddr32 = (lane ^ 32) << 2;
    const int nktile = k_JB >> 4;
    const int ntile_chunk = k_chunk >> 4;
    bool table_ready = false;
    // FP32 screen (V16): a tile group's distances first by FP32 MFMAs (v_mfma_f32_16x16x4f32,
    // a third of the FP64 instruction's cycles); the FP64 group runs only if some entry can be
    // within the skip bound.  |d32 - d| <= 2^-17 (2 max_i alpha_i + gamma_k) (rounding of the
    // operands and of K2 + 1 f32 sums, |sum_kk P' Q| <= 2 |p_i||q_k| <= alpha_i + gamma_k), so
    // a screened-out group is one the FP64 test below would discard too: results are bitwise
    // those of the unscreened sweep.  A symbol whose groups mostly pass (wide posterior) stops
    // screening after 16 groups.
    double amax = 0.0;               // max_i alpha_i (set with the alpha table)
    bool scr_on = V16 && c.screen;   // wave-uniform
    int scr_n = 0, scr_pass = 0;

    // Per-group bounds (V16).  The column-tile and row-tile bounds above each relax TWO streams
    // to the continuum; at theta_0's ill-conditioned H_eff that is loose and most tile groups
    // reach the screen only to be rejected there.  Relaxing ONE stream q (P_q = I - h_q h_q^H /
    // ||h_q||^2, so P_q h_q = 0 and ||P_q v|| <= ||v||) bounds every hypothesis of the tile group
    // G(kt, tg) (x_2 = cons[kt], x_0 in cons[tg .. tg+3], every x_1 and x_3) from below by
    //   T_3 = min over x_0 in the block and x_1 of ||P_3 (y - h_0 x_0 - h_1 x_1 - h_2 x_2)||^2
    //   T_1 = min over x_0 in the block and x_3 of ||P_1 (y - h_0 x_0 - h_3 x_3 - h_2 x_2)||^2.
    // Each has the sweep's own form alpha'_i + gamma'_k - 2 Re p'_i^H q'_k with 256 rows
    // (x_0, x_o), o = 1 or 3 (A operand U'_{x_0} + V'_{x_o}) and 16 columns x_2: per bound 16
    // tiles of STEPS FP32 MFMAs and STEPS more for alpha', reduced to the 4 x 16 group table by an
    // element-wise minimum over the four tiles of an x_0 block, the four rows of the lane and two
    // cross-lane steps.  Lane (rq, col) keeps the bound of group (tg = 4 rq, kt = col):
    // max(T_3, T_1), each less its rounding margin
    //   2^-16 (2 A' + gamma'_kt) + 1e-9 S,   A' = 2 (max ||P(y - h_0 x)||^2 + max ||P h_o x||^2)
    //   >= max alpha',   S = 4 (||y||^2 + max |x|^2 sum_a ||h_a||^2), of the order of the largest
    //   distance (five terms: 5/4 S bounds every one; S only scales the 1e-9 term):
    // the first term is the screen's 2^-17 (2 max alpha + gamma) (operands and alpha' rounded to
    // FP32, K2 + 1 FP32 sums) doubled for alpha' being formed in FP32 as well, the second covers
    // the FP64 projection (P_q h_q = 0 only to rounding) and the sweep's own FP64 rounding, as
    // lb_margin does for the column bounds.  A group whose bound exceeds the skip bound holds no
    // hypothesis the FP64 test would keep, so skipping it leaves every result bit as it was.
    // ||h_q||^2 = 0, a column below 1e-20 of the largest, or a scale outside FP32's range leave
    // that bound at 0, which skips nothing.  The projected vectors are formed here from H and y
    // (the prep record has no room for them).
    double tri_lane = 0.0;
    bool tri_have = false;           // wave-uniform: the group table of this symbol is built
    auto build_tri = [&]() {
        float* tU = s_U32 + 256;
        float* tV = tU + 64 * STEPS;
        float* tQ = tV + 64 * STEPS;
        float* tA = tQ + 64 * STEPS;                        // alpha', after the projected vectors
        cd* pv = reinterpret_cast<cd*>(tA);                 // [4][8]: P y, P h_0, P h_o, P h_2
        const int r = lane & 7, vi = (lane >> 3) & 3;
        const bool own = r < NR;
        const cd* yv = prep ? reinterpret_cast<const cd*>(s_rec + k_prep_stride)
                            : a.yd + (size_t)gsym * NR;
        const int xa4 = (lane ^ 4) << 2, xa2 = (lane ^ 2) << 2, xa1 = (lane ^ 1) << 2;
        auto rsum = [&](double v) {                         // sum over the 8-lane group
            v += bperm_d(v, xa4);
            v += bperm_d(v, xa2);
            return v + bperm_d(v, xa1);
        };
        const double cmax2 = wave_max_dpp(cabs2(s_cons[col]));
        double hh = 0.0;                                    // ||h_a||^2 of the lane's column a = vi
        hh = rsum(own ? cabs2(H[vi * NR + r]) : 0.0);
        const double hmax = wave_max_dpp(hh);
        const double hsum = (lane_d(hh, 0) + lane_d(hh, 8)) + (lane_d(hh, 16) + lane_d(hh, 24));
        const double y2 = lane_d(rsum(own ? cabs2(yv[r]) : 0.0), 0);
        const double S = 4.0 * fma(cmax2, hsum, y2);
        const bool range_ok = S > 1e-30 && S < 1e30;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const int q = pass ? 1 : 3, o = pass ? 3 : 1;
            const cd hq = own ? H[q * NR + r] : czero();
            const cd v = own ? (vi == 0 ? yv[r] : H[(vi == 1 ? 0 : (vi == 2 ? o : 2)) * NR + r]) : czero();
            const double hq2 = rsum(cabs2(hq));
            const bool ok = range_ok && hq2 > 0.0 && hq2 >= 1e-20 * hmax;
            if (!__all(ok)) continue;
            const cd cf = cscale(cmk(rsum(fma(hq.x, v.x, hq.y * v.y)), rsum(fma(hq.x, v.y, -hq.y * v.x))),
                                 1.0 / hq2);               // h_q^H v / ||h_q||^2
            const cd pvv = csub(v, cmul(hq, cf));
            wave_sync();                                    // the other pass has read alpha'
            if (lane < 32) pv[vi * 8 + r] = own ? pvv : czero();
            wave_sync();
            double uu = 0.0, vv = 0.0, qq = 0.0;
#pragma unroll
            for (int it = 0; it < STEPS; ++it) {
                const int kk = 4 * it + rq, e = kk * 16 + col;
                double u = 0.0, w = 0.0, q2 = 0.0;
                if (kk < K2) {
                    const int rr = kk >> 1;
                    const cd x = s_cons[col];
                    const cd pu = csub(pv[rr], cmul(pv[8 + rr], x));
                    const cd hv = cmul(pv[16 + rr], x);
                    const cd hx = cmul(pv[24 + rr], x);
                    u = -2.0 * ((kk & 1) ? pu.y : pu.x);
                    w = 2.0 * ((kk & 1) ? hv.y : hv.x);
                    q2 = (kk & 1) ? hx.y : hx.x;
                }
                tU[e] = (float)u;
                tV[e] = (float)w;
                tQ[e] = (float)q2;
                uu = fma(u, u, uu);
                vv = fma(w, w, vv);
                qq = fma(q2, q2, qq);
            }
            // |U'_x|^2, |V'_x|^2 and gamma'_x = ||q'_x||^2 of x = cons[col], in every lane of the column
            uu += bperm_d(uu, xaddr16); uu += bperm_d(uu, xaddr32);
            vv += bperm_d(vv, xaddr16); vv += bperm_d(vv, xaddr32);
            qq += bperm_d(qq, xaddr16); qq += bperm_d(qq, xaddr32);
            const double amaxp = 0.5 * (wave_max_dpp(uu) + wave_max_dpp(vv));
            const double margin = fma(0x1p-16, 2.0 * amaxp + qq, 1e-9 * S);
            wave_sync();                                    // tables written, pv read
            // alpha'[s0][s1] = 0.25 (|U'_s0|^2 + |V'_s1|^2) + 0.5 U'_s0 . V'_s1, the cross terms
            // by STEPS MFMAs: this lane's values are rows s0 = 4 rq + j, column s1 = col
            float vr32[STEPS], qr32[STEPS];
            f4v cx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                vr32[s] = tV[(4 * s + rq) * 16 + col];
                qr32[s] = tQ[(4 * s + rq) * 16 + col];
                cx = __builtin_amdgcn_mfma_f32_16x16x4f32(tU[(4 * s + rq) * 16 + col], vr32[s], cx, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double us = bperm_d(uu, (4 * rq + j) << 2);
                tA[(4 * rq + j) * 16 + col] = (float)fma(0.5, (double)cx[j], 0.25 * (us + vv));
            }
            wave_sync();
            double tq = 0.0;
#pragma unroll 1
            for (int blk = 0; blk < 4; ++blk) {
                f4v t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    t[u] = *reinterpret_cast<const f4v*>(tA + (4 * blk + u) * 16 + rq * 4);
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        t[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            tU[(4 * s + rq) * 16 + 4 * blk + u] + vr32[s], qr32[s], t[u], 0, 0, 0);
                float mm = fminf(fminf(t[0][0], t[0][1]), fminf(t[0][2], t[0][3]));
#pragma unroll
                for (int u = 1; u < 4; ++u)
                    mm = fminf(mm, fminf(fminf(t[u][0], t[u][1]), fminf(t[u][2], t[u][3])));
                mm = fminf(mm, __int_as_float(__builtin_amdgcn_ds_bpermute(xaddr16, __float_as_int(mm))));
                mm = fminf(mm, __int_as_float(__builtin_amdgcn_ds_bpermute(xaddr32, __float_as_int(mm))));
                if (rq == blk) tq = ((double)mm + qq) - margin;
            }
            tri_lane = fmax(tri_lane, tq);
        }
    };

    const double hard_bound = d0 + 1e-10 * cscale_d + 1e-300;
    unsigned groups = 0;             // wave-uniform count of issued tile groups
    // TP: bit 4 kt + row block of every group that passed the search's FP64 test (wave-uniform)
    [[maybe_unused]] unsigned long long hit = 0;
    unsigned reached = 0;            // ... and of tile groups that reached the screen
    // Best-first order (V16, soft).  The running minimum starts at the ridge-rounded candidate,
    // a poor hypothesis at theta_0's ill-conditioned H_eff, and every group met before the true
    // minimum is tested against a loose skip bound.  So the 16 column tiles are visited by
    // ascending column-tile bound and, inside one, the four row blocks by ascending minimum of
    // their row-tile bounds: the tiles that can hold the minimum come first.  Both bounds exist
    // before the sweep and depend on no switch, a skipped group holds nothing the posterior
    // keeps, so the moments change in summation order alone.  Ties keep the smaller index (all
    // bounds equal, or all below their rounding margin as at n_rx <= 2, is the natural order).
    // The hard decision is "the first minimum in product order" and keeps the natural order.
    // The order is wave-uniform: 16 nibbles (kt at position n) and 4 x 2 bits (block at
    // position n), in scalar registers.
    constexpr bool ORD = V16 && MODE != SBCE_ESTEP_HARD;
    const bool ordered = ORD && (SBCE_AB ? c.order != 0 : true);
    unsigned long long ktord = 0xfedcba9876543210ull;
    if constexpr (ORD) {
        if (ordered) {
            // a bound below its own rounding margin says nothing (n_rx <= 2: P = 0 up to
            // rounding): such bounds tie at 0 and keep the natural order among themselves
            const double lbc = lbp[col];
            const double mine = lbc < lb_margin ? 0.0 : lbc;
            int rank = 0;            // tiles in front of tile `col`: smaller bound, or equal and smaller index
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double lbj = lbp[j];
                const double o = lbj < lb_margin ? 0.0 : lbj;
                rank += (o < mine || (o == mine && j < col)) ? 1 : 0;
            }
            // the ranks are a permutation: tile col goes to nibble `rank`; OR over the 16 lanes
            // of a row (every row computes the same) by DPP, as wave_min_dpp reduces
            const unsigned nib = (unsigned)col << ((rank & 7) << 2);
            unsigned lo = rank < 8 ? nib : 0u, hi = rank < 8 ? 0u : nib;
            auto row_or = [](unsigned v) {
                v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
                v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
                v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
                v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
                return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
            };
            lo = row_or(lo);
            hi = row_or(hi);
            ktord = ((unsigned long long)hi << 32) | lo;
        }
    }
    // column tiles whose exact bound (column_tile_bounds) admits the skip bound as it stands
    // now; the bound only falls during the sweep, so each is checked again when reached
    [[maybe_unused]] unsigned long long ktmask = ~0ull;
    if (!ORD && nktile <= 64) {
        const double lim0 = ((MODE == SBCE_ESTEP_HARD) ? hard_bound : mshift + thr_d) + lb_margin;
        ktmask = __ballot(lane < nktile && !(lbp[lane < nktile ? lane : 0] > lim0));
    }
    // (kn: the position in the order, which sets kt; the natural sweep counts kt itself)
    for (int kt = 0, kn = 0; (ORD ? kn : kt) < nktile; ++kt, ++kn) {
        if constexpr (ORD) {
            kt = (int)(ktord >> (4 * kn)) & 15;
        } else if (nktile <= 64) {
            const unsigned long long m = ktmask >> kt;
            if (!m) break;
            kt += __builtin_ctzll(m);
        }
        // exact column-tile bound: wave-uniform skip of the whole tile (best-first: the bounds
        // ascend and the skip bound only falls, so the first tile above it ends the symbol)
        if (lbp[kt] > ((MODE == SBCE_ESTEP_HARD) ? hard_bound : mshift + thr_d) + lb_margin) {
            if (ORD && ordered) break;
            continue;
        }
        unsigned rowmask = 0xffffu;
        [[maybe_unused]] unsigned blkord = 0xe4u;    // row blocks 0, 1, 2, 3
        if constexpr (V16) {
            // per-group bounds: built once kTriGate groups of the symbol have reached the screen
            // (the later E-steps' symbols, with a group or two left, never pay for the tables);
            // a column tile whose four groups are all dead is left before its setup
            if (c.tri && !tri_have && (c.tri == 2 || reached >= kTriGate)) {
                build_tri();
                tri_have = true;
            }
            if (tri_have) {
                const double lim = (MODE == SBCE_ESTEP_HARD) ? hard_bound : mshift + thr_d;
                const unsigned long long lv = __ballot(tri_lane <= lim) >> kt;   // bit 16 blk: group alive
                rowmask = ((lv & 1) ? 0x000fu : 0u) | ((lv >> 16 & 1) ? 0x00f0u : 0u) |
                          ((lv >> 32 & 1) ? 0x0f00u : 0u) | ((lv >> 48 & 1) ? 0xf000u : 0u);
            }
        }
        unsigned rowlive = 0xffffu;                      // row tiles the row-tile bound admits
        double bnd = INFINITY;
        if (rowb) {
            if (lane < 16) {
                const cd x0 = s_cons[lane];
                const double* rk = s_rk + 3 * kt;
                bnd = fma(cabs2(x0), s_tab[63], rk[0] - 2.0 * (x0.x * rk[1] + x0.y * rk[2]));
            }
            const double lim = ((MODE == SBCE_ESTEP_HARD) ? hard_bound : mshift + thr_d) + lb_margin;
            rowlive = (unsigned)__ballot(bnd <= lim);
        }
        if constexpr (V16) {
            // A group the row bound admits and the per-group bound rejects is one the screen would
            // have rejected: it counts in the screen's pass rate, so that the screen stops for the
            // same symbols with and without the per-group bounds (these never add an FP64 group).
            if (tri_have && scr_on) {
                unsigned rl = rowlive | (rowlive >> 1);
                rl |= rl >> 2;                           // bit 4 blk: a row tile of the block is admitted
                scr_n += __builtin_popcount(rl & ~rowmask & 0x1111u);
            }
        }
        rowmask &= rowlive;
        if (!rowmask) continue;                          // no group of this column tile survives
        if constexpr (ORD) {
            if (rowb && ordered) {
                // block minimum of the row bounds (lanes 4 blk .. 4 blk + 3), ranked as above
                double bm = fmin(bnd, dpp_d<0xB1>(bnd));
                bm = fmin(bm, dpp_d<0x4E>(bm));
                bm = bm < lb_margin ? 0.0 : bm;
                const int blk = (lane >> 2) & 3;
                int rank = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double o = lane_d(bm, 4 * j);
                    rank += (o < bm || (o == bm && j < blk)) ? 1 : 0;
                }
                const int code = blk << (2 * rank);
                blkord = (unsigned)(__builtin_amdgcn_readlane(code, 0) | __builtin_amdgcn_readlane(code, 4) |
                                    __builtin_amdgcn_readlane(code, 8) | __builtin_amdgcn_readlane(code, 12));
            }
        }
        const int k = kt * 16 + col;
        cd xb[NB];
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) xb[bb] = s_cons[(k >> (k_lm * (NB - 1 - bb))) & mask];
        double bop[STEPS];
        float bop32[STEPS];
        double gam = 0.0;
        if constexpr (V16) {
            // gamma_k = ||q_k||^2 = sum over the 4 lanes of column k of their bop^2
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                bop[s] = s_Q2[(4 * s + rq) * 16 + kt] + q3reg[s];
                gam = fma(bop[s], bop[s], gam);
            }
            gam += bperm_d(gam, xaddr16);
            gam += bperm_d(gam, xaddr32);
#pragma unroll
            for (int s = 0; s < STEPS; ++s) bop32[s] = (float)bop[s];
        } else {
            cd qv[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                cd acc = czero();
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) acc = cfma(acc, H[(NA + bb) * NR + r], xb[bb]);
                qv[r] = acc;
                gam += cabs2(acc);
            }
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int kk = 4 * s + rq;
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (kk == 2 * r) v = qv[r].x;
                    if (kk == 2 * r + 1) v = qv[r].y;
                }
                bop[s] = v;
            }
        }
        double ck = 0.0;
        cd mu[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) mu[q] = czero();
        bool touched = false;       // wave-uniform: an exp was taken in this column tile
        // V16 (NA = 2): hypothesis i = 16 s0 + s1 with s0 = the tile (wave-uniform per tile) and
        // s1 = rq + 4 j (the lane's row j), so the per-column-tile sums factor: R1[j] = sum over
        // tiles of w (-> ck, mu_1, nu_1), Q[j] = sum of w x_s0 (-> mu_0, and kappa through
        // conj(x_s1)), N0 = sum of w |x_s0|^2 (-> nu_0); 4 VALU ops per weight instead of 21,
        // the x_s1 products once per column tile
        double R1[4] = {0.0, 0.0, 0.0, 0.0}, N0 = 0.0;
        cd Q[4] = {czero(), czero(), czero(), czero()};

        for (int i0 = 0; i0 < k_JA; i0 += k_chunk) {
            if (!table_ready && V16) {
                // ---- alpha[s0*16 + s1] = 0.25 ||U_s0 + V_s1||^2
                //      = 0.25 (|U_s0|^2 + |V_s1|^2) + 0.5 U_s0 . V_s1: the cross terms are a
                //      16 x 16 x K2 real GEMM (STEPS MFMAs, B operand = vreg); stored as
                //      s_al[s0*16 + (s1 & 3)*4 + (s1 >> 2)] so that a tile's accumulator init
                //      (rows rq + 4j) is two 16-byte reads ----
                wave_sync();
                double nrm = 0.0;
                const double* T = lane < 16 ? s_U : s_V;
#pragma unroll
                for (int kk = 0; kk < K2; ++kk) {
                    const double v = T[kk * 16 + (lane & 15)];
                    nrm = fma(v, v, nrm);
                }
                if (lane < 32) s_tab[lane] = nrm;
                mf4 cx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
                    cx = __builtin_amdgcn_mfma_f64_16x16x4f64(s_U[(4 * s + rq) * 16 + col], vreg[s],
                                                              cx, 0, 0, 0);
                wave_sync();
                const double nvv = s_tab[16 + col];
                double am = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s0 = rq + 4 * j;
                    const double al = 0.25 * (s_tab[s0] + nvv) + 0.5 * cx[j];
                    s_al[s0 * 16 + (col & 3) * 4 + (col >> 2)] = al;
                    s_al32[s0 * 16 + col] = (float)al;     // natural order: f32 C/D rows 4 rq + q
                    am = fmax(am, al);
                }
                amax = wave_max_dpp(am);
                wave_sync();
                table_ready = true;
            }
            if (!table_ready) {
                // ---- alpha_i = ||p_i||^2 for entries i0 .. i0+chunk-1 from U, V ----
                wave_sync();
                for (int e = lane; e < k_chunk; e += 64) {
                    const int i = i0 + e;
                    const int su = (NA == 2) ? (i >> k_lm) : i;
                    const int sv = i & mask;
                    double al = 0.0;
#pragma unroll
                    for (int kk = 0; kk < K2; ++kk) {
                        double v = s_U[kk * k_M + su];
                        if (NA == 2) v += s_V[kk * k_M + sv];
                        al = fma(v, v, al);
                    }
                    s_al[e] = 0.25 * al;
                }
                wave_sync();
                table_ready = (k_JA == k_chunk);
            }
            for (int tg = 0, tn = 0; (ORD ? tn : tg) < ntile_chunk; tg += TU, tn += TU) {
                // TU independent 16x16 tiles in flight: STEPS*TU MFMAs per group;
                // accumulators start at alpha_i, gamma_k (lane constant) stays outside
                if constexpr (ORD) tg = (int)((blkord >> (tn >> 1)) & 3u) << 2;   // TU = 4: position tn / 4
                if (V16 && !((rowmask >> tg) & ((1u << TU) - 1u))) continue;
                if constexpr (V16) {
                    // again as the group is reached (the skip bound falls inside a column tile
                    // too; hard: the lanes' own running minima)
                    const bool dead = tri_have && !__any(lane_d(tri_lane, kt + 4 * tg) <=
                                                         ((MODE == SBCE_ESTEP_HARD) ? best_d : mshift + thr_d));
                    scr_n += (int)(dead & scr_on);
                    if (dead) continue;
                }
                ++reached;
                if (V16 && scr_on) {
                    f4v s32[TU];
#pragma unroll
                    for (int u = 0; u < TU; ++u)
                        s32[u] = *reinterpret_cast<const f4v*>(s_al32 + (tg + u) * 16 + rq * 4);
#pragma unroll
                    for (int s = 0; s < STEPS; ++s)
#pragma unroll
                        for (int u = 0; u < TU; ++u) {
                            const float av = s_U32[(4 * s + rq) * 16 + (i0 >> 4) + tg + u] + vreg32[s];
                            s32[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bop32[s], s32[u], 0, 0, 0);
                        }
                    float m32 = fminf(fminf(s32[0][0], s32[0][1]), fminf(s32[0][2], s32[0][3]));
#pragma unroll
                    for (int u = 1; u < TU; ++u)
                        m32 = fminf(m32, fminf(fminf(s32[u][0], s32[u][1]), fminf(s32[u][2], s32[u][3])));
                    const double lim = ((MODE == SBCE_ESTEP_HARD) ? best_d : mshift + thr_d) - gam +
                                       0x1p-17 * (2.0 * amax + gam);
                    ++scr_n;
                    const bool pass = __any((double)m32 <= lim);
                    scr_pass += pass;
                    if (scr_n >= 16 && 2 * scr_pass > scr_n) scr_on = false;
                    if (!pass) continue;
                }
                ++groups;
                mf4 acc[TU];
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    if (V16) {            // rows rq + 4j of tile tg + u: 4 consecutive doubles
                        const cd lo = *reinterpret_cast<const cd*>(s_al + (tg + u) * 16 + rq * 4);
                        const cd hi = *reinterpret_cast<const cd*>(s_al + (tg + u) * 16 + rq * 4 + 2);
                        acc[u] = mf4{lo.x, lo.y, hi.x, hi.y};
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[u][j] = s_al[(tg + u) * 16 + rq + 4 * j];
                    }
                }
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
#pragma unroll
                    for (int u = 0; u < TU; ++u) {
                        const int kk = 4 * s + rq;
                        double av;
                        if (V16) {
                            av = s_U[kk * 16 + (i0 >> 4) + tg + u] + vreg[s];
                        } else {
                            const int ia = i0 + (tg + u) * 16 + col;      // A-operand row
                            av = s_U[kk * k_M + ((NA == 2) ? (ia >> k_lm) : ia)];
                            if (NA == 2) av += s_V[kk * k_M + (ia & mask)];
                        }
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bop[s], acc[u], 0, 0, 0);
                    }
                double cm = fmin(fmin(acc[0][0], acc[0][1]), fmin(acc[0][2], acc[0][3]));
#pragma unroll
                for (int u = 1; u < TU; ++u)
                    cm = fmin(cm, fmin(fmin(acc[u][0], acc[u][1]), fmin(acc[u][2], acc[u][3])));
                // one comparison per tile group (soft: within thr of the shift, hard: not
                // worse than this lane's best); the common case skips everything below
                if (MODE == SBCE_ESTEP_HARD) {
                    if (!__any(cm + gam <= best_d)) continue;
                } else if (!__any(cm + gam <= mshift + thr_d)) {
                    continue;
                }
                if constexpr (TP) {
                    // the search keeps the running minimum (the same sequence of values as the
                    // one-pass sweep, so every skip decision is that sweep's) and marks the group
                    cm += gam;
                    if (__any(cm < mshift)) mshift = wave_min_dpp(fmin(cm, mshift));
                    hit |= 1ull << (4 * kt + (tg >> 2));
                    continue;
                }
                if (MODE == SBCE_ESTEP_HARD) {
                    const double lim = best_d - gam;
#pragma unroll
                    for (int u = 0; u < TU; ++u)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double dv = acc[u][j];
                            if (dv <= lim) {
                                const int jj = (i0 + (tg + u) * 16 + rq + 4 * j) * k_JB + k;
                                const double dd = dv + gam;
                                if (dd < best_d || (dd == best_d && jj < best_j)) { best_d = dd; best_j = jj; }
                            }
                        }
                    continue;
                }
                cm += gam;
                if (__any(cm < mshift)) {
                    double mn = fmin(cm, mshift);
                    mn = wave_min_dpp(mn);
                    const double f = fexp_neg((mn - mshift) * inv_s2);
                    mshift = mn;
                    // V16: ck, mu are formed at the column tile's end; the stream-3 totals
                    // (x_3 = cons[col], a lane constant) are formed after the sweep
                    constexpr int NBS = V16 ? 1 : NB;
                    tot_c *= f; kap = cscale(kap, f);
                    if constexpr (!V16) { ck *= f; tot_kB = cscale(tot_kB, f); }
#pragma unroll
                    for (int q = 0; q < NA; ++q) {
                        tot_muA[q] = cscale(tot_muA[q], f); nu[q] *= f;
                        if constexpr (!V16) mu[q] = cscale(mu[q], f);
#pragma unroll
                        for (int bb = 0; bb < NBS; ++bb) tot_X[q][bb] = cscale(tot_X[q][bb], f);
                    }
#pragma unroll
                    for (int bb = 0; bb < NBS; ++bb) { tot_mB[bb] = cscale(tot_mB[bb], f); tot_nB[bb] *= f; }
                    if constexpr (V16) {
                        N0 *= f;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { R1[j] *= f; Q[j] = cscale(Q[j], f); }
                    }
                }
                if (!__any(cm <= mshift + thr_d)) continue;
                touched = true;
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const double cmu =
                        fmin(fmin(acc[u][0], acc[u][1]), fmin(acc[u][2], acc[u][3])) + gam;
                    if (!__any(cmu <= mshift + thr_d)) continue;
                    if constexpr (V16) {
                        const cd x0 = s_cons[tg + u];          // stream 0 of the tile (i0 = 0)
                        const double n0 = cabs2(x0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double dj = acc[u][j] + gam;
                            // rows with no lane inside the bound: weights < e^-50 of the maximum
                            if (!__any(dj <= mshift + thr_d)) continue;
                            const double w = fexp_neg((mshift - dj) * inv_s2);
                            R1[j] += w;
                            Q[j] = caxpy(Q[j], w, x0);
                            N0 = fma(w, n0, N0);
                        }
                        continue;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = i0 + (tg + u) * 16 + rq + 4 * j;
                        const double w = fexp_neg((mshift - (acc[u][j] + gam)) * inv_s2);
                        cd xa[NA];
#pragma unroll
                        for (int q = 0; q < NA; ++q) xa[q] = s_cons[(i >> (k_lm * (NA - 1 - q))) & mask];
                        ck += w;
#pragma unroll
                        for (int q = 0; q < NA; ++q) {
                            mu[q] = caxpy(mu[q], w, xa[q]);
                            nu[q] = fma(w, cabs2(xa[q]), nu[q]);
                        }
                        if (NPA) kap = caxpy(kap, w, cmulc(xa[0], xa[NA > 1 ? 1 : 0]));
                    }
                }
            }
        }
        if (!TP && MODE == SBCE_ESTEP_SOFT && touched) {
            if constexpr (V16) {
                // the lane's row streams x_s1 = cons[rq + 4 j]
                ck = (R1[0] + R1[1]) + (R1[2] + R1[3]);
                mu[0] = cadd(cadd(Q[0], Q[1]), cadd(Q[2], Q[3]));
                mu[1] = czero();
                nu[0] += N0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const cd x1 = s_cons[rq + 4 * j];
                    mu[1] = caxpy(mu[1], R1[j], x1);
                    nu[1] = fma(R1[j], cabs2(x1), nu[1]);
                    kap = cadd(kap, cmulc(Q[j], x1));
                }
            }
            constexpr int NBS = V16 ? 1 : NB;
            tot_c += ck;
#pragma unroll
            for (int bb = 0; bb < NBS; ++bb) {
                tot_mB[bb] = caxpy(tot_mB[bb], ck, xb[bb]);
                tot_nB[bb] = fma(ck, cabs2(xb[bb]), tot_nB[bb]);
            }
            if (NPB && !V16) tot_kB = caxpy(tot_kB, ck, cmulc(xb[0], xb[NB > 1 ? 1 : 0]));
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                tot_muA[q] = cadd(tot_muA[q], mu[q]);
#pragma unroll
                for (int bb = 0; bb < NBS; ++bb) tot_X[q][bb] = cfmac(tot_X[q][bb], mu[q], xb[bb]);
            }
        }
    }
    // Second pass (TP).  The search above held no posterior sum: the 25 lane totals and the
    // per-column-tile R1 / Q / N0 are live only from here on, which is what lets the search run at
    // three waves per SIMD.  The minimum d_min = mshift is final, so the weights are
    // exp((d_min - d) / s^2) directly and nothing is ever rescaled.  The marked groups are visited
    // in natural order (kt ascending, row block ascending), whatever order the search took; each
    // is recomputed tile by tile with the same FP64 MFMAs on the same operands (bitwise the
    // search's distances), and a tile that holds nothing within d_min + thr_d (its group was
    // marked under an earlier, looser minimum, or by another tile) is dropped.  The sums are the
    // one-pass sweep's factored ones.
    [[maybe_unused]] unsigned groups2 = 0;           // wave-uniform count of recomputed groups
    if constexpr (TP) {
        for (unsigned long long left = hit; left;) {
            const int kt = __builtin_ctzll(left) >> 2;
            const unsigned blks = (unsigned)(left >> (4 * kt)) & 15u;
            left &= ~(15ull << (4 * kt));
            double bop[STEPS];
            double gam = 0.0;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                bop[s] = s_Q2[(4 * s + rq) * 16 + kt] + q3reg[s];
                gam = fma(bop[s], bop[s], gam);
            }
            gam += bperm_d(gam, xaddr16);
            gam += bperm_d(gam, xaddr32);
            double R1[4] = {0.0, 0.0, 0.0, 0.0}, N0 = 0.0;
            cd Q[4] = {czero(), czero(), czero(), czero()};
            bool touched = false;
            groups2 += __builtin_popcount(blks);
            // one tile at a time (marked groups are few; the search's registers set the allocation)
#pragma unroll 1
            for (int tl = 0; tl < 16; ++tl) {
                if (!((blks >> (tl >> 2)) & 1u)) continue;
                const cd lo = *reinterpret_cast<const cd*>(s_al + tl * 16 + rq * 4);
                const cd hi = *reinterpret_cast<const cd*>(s_al + tl * 16 + rq * 4 + 2);
                mf4 acc = mf4{lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_U[(4 * s + rq) * 16 + tl] + vreg[s], bop[s],
                                                               acc, 0, 0, 0);
                const double cmu = fmin(fmin(acc[0], acc[1]), fmin(acc[2], acc[3])) + gam;
                if (!__any(cmu <= mshift + thr_d)) continue;
                touched = true;
                const cd x0 = s_cons[tl];                      // stream 0 of the tile
                const double n0 = cabs2(x0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dj = acc[j] + gam;
                    // rows with no lane inside the bound: weights < e^-50 of the maximum
                    if (!__any(dj <= mshift + thr_d)) continue;
                    const double w = fexp_neg((mshift - dj) * inv_s2);
                    R1[j] += w;
                    Q[j] = caxpy(Q[j], w, x0);
                    N0 = fma(w, n0, N0);
                }
            }
            if (!touched) continue;
            // the column tile's sums into the totals, as the one-pass sweep folds them
            const cd x2 = s_cons[kt];                          // stream 2 of the column tile
            const double ck = (R1[0] + R1[1]) + (R1[2] + R1[3]);
            cd mu[NA];
            mu[0] = cadd(cadd(Q[0], Q[1]), cadd(Q[2], Q[3]));
            mu[1] = czero();
            nu[0] += N0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const cd x1 = s_cons[rq + 4 * j];
                mu[1] = caxpy(mu[1], R1[j], x1);
                nu[1] = fma(R1[j], cabs2(x1), nu[1]);
                kap = cadd(kap, cmulc(Q[j], x1));
            }
            tot_c += ck;
            tot_mB[0] = caxpy(tot_mB[0], ck, x2);
            tot_nB[0] = fma(ck, cabs2(x2), tot_nB[0]);
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                tot_muA[q] = cadd(tot_muA[q], mu[q]);
                tot_X[q][0] = cfmac(tot_X[q][0], mu[q], x2);
            }
        }
    }
    if constexpr (V16) {
        // stream 3 is the lane constant x_3 = cons[col] (k = 16 kt + col): its sums are the
        // lane's totals times x_3
        const cd x3 = s_cons[col];
        tot_mB[1] = cscale(x3, tot_c);
        tot_nB[1] = tot_c * cabs2(x3);
        tot_kB = cmulc(tot_mB[0], x3);
#pragma unroll
        for (int q = 0; q < NA; ++q) tot_X[q][1] = cmulc(tot_muA[q], x3);
    }

    if (c.count && lane == 0) {
        atomicAdd(&g_estep_mfma, (unsigned long long)groups * STEPS * TU);
        if (V16) atomicAdd(&g_estep_groups, (unsigned long long)reached);
        if (TP) atomicAdd(&g_estep_pass2, (unsigned long long)groups2);
    }
    constexpr int MS = NT + NT * NT;
    cd* out = a.mom + (size_t)gsym * MS;
    // The moment-repeat fold (armed by a.mchg): the lane that stores output word `lane` loads the
    // word it overwrites ahead of the reduction and compares the bit patterns at the store.
    const bool arm = a.mchg != nullptr;
    cd mold = czero();
    if (arm && lane < MS) mold = out[lane];
    if (MODE == SBCE_ESTEP_HARD) {
        wave_argmin_dpp(best_d, best_j);
        if (lane < MS) {                       // lane o writes output o (m_t, then S_t row-major)
            const int s2 = lane < NT ? lane : (lane - NT) / NT;
            const int s3 = lane < NT ? 0 : (lane - NT) % NT;
            const cd xp = s_cons[(best_j >> (k_lm * (NT - 1 - s2))) & mask];
            const cd xq = s_cons[(best_j >> (k_lm * (NT - 1 - s3))) & mask];
            const cd mv = mom_word(lane < NT ? xp : cmulc(xp, xq));
            out[lane] = mv;
            if (arm && mom_bits_differ(mold, mv)) a.mchg[b] = 1;
        }
        return;
    }
    int xa[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) xa[i] = (lane ^ (32 >> i)) << 2;
    {
        // Reduce-scatter by recursive halving: at the step with lane offset o a lane keeps the
        // half of the remaining values selected by its bit o and receives the partner's copy
        // of that half (32 + 16 + ... doubles moved instead of 6 per value); value j ends in
        // the lanes whose bits 5..1 spell j, and is gathered through LDS.
        constexpr int NV = 1 + 2 * NPA + 2 * NPB + 3 * NA + 2 * NA * NB + 3 * NB;
        static_assert(NV <= 32, "reduce-scatter holds at most 32 values");
        double v[32];
        int n = 0;
        auto put = [&](double x) { v[n++] = x; };
        put(tot_c);
        if (NPA) { put(kap.x); put(kap.y); }
        if (NPB) { put(tot_kB.x); put(tot_kB.y); }
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            put(tot_muA[q].x); put(tot_muA[q].y); put(nu[q]);
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) { put(tot_X[q][bb].x); put(tot_X[q][bb].y); }
        }
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) { put(tot_mB[bb].x); put(tot_mB[bb].y); put(tot_nB[bb]); }
#pragma unroll
        for (int i = NV; i < 32; ++i) v[i] = 0.0;
#pragma unroll
        for (int st = 0; st < 5; ++st) {
            const int h = 16 >> st;
            const bool hi = (lane >> (5 - st)) & 1;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const double snd = hi ? v[i] : v[h + i];
                const double kp = hi ? v[h + i] : v[i];
                v[i] = kp + bperm_d(snd, xa[st]);
            }
        }
        v[0] += bperm_d(v[0], xa[5]);
        double* red = s_tab;                 // wave scratch (>= 32 doubles)
        const int j = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 +
                      ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
        wave_sync();
        if (!(lane & 1)) red[j] = v[0];
        wave_sync();
        // lane o < NT + NT^2 writes output o (m_t, then S_t row-major) from the gathered
        // totals: numerator at red[ire] (+ i red[iim]), conjugated when cj, times 1/Z
        if (lane < NT + NT * NT) {
            constexpr int OFF_KA = 1, OFF_KB = 1 + 2 * NPA;
            constexpr int BQ = 1 + 2 * NPA + 2 * NPB, SQ = 3 + 2 * NB;
            constexpr int BB = BQ + NA * SQ;
            int ire, iim = -1;
            bool cj = false;
            if (lane < NT) {
                ire = lane < NA ? BQ + lane * SQ : BB + 3 * (lane - NA);
                iim = ire + 1;
            } else {
                const int i = (lane - NT) / NT, j = (lane - NT) - (lane - NT) / NT * NT;
                if (i == j) {
                    ire = i < NA ? BQ + i * SQ + 2 : BB + 3 * (i - NA) + 2;
                } else if (i < NA && j < NA) {
                    ire = OFF_KA; iim = OFF_KA + 1; cj = i > j;
                } else if (i >= NA && j >= NA) {
                    ire = OFF_KB; iim = OFF_KB + 1; cj = i > j;
                } else if (i < NA) {
                    ire = BQ + i * SQ + 3 + 2 * (j - NA); iim = ire + 1;
                } else {
                    ire = BQ + j * SQ + 3 + 2 * (i - NA); iim = ire + 1; cj = true;
                }
            }
            const double iz = 1.0 / red[0];
            const double re = red[ire], im = iim >= 0 ? red[iim] : 0.0;
            const cd mv = mom_word(cmk(re * iz, (cj ? -im : im) * iz));
            out[lane] = mv;
            if (arm && mom_bits_differ(mold, mv)) a.mchg[b] = 1;
        }
    }
    }();
    }
    if (!listed) return;
    }
}

template <int NT, int NR, int MODE, int TU, bool V16 = false>
__global__ __launch_bounds__(128) void estep_mfma_kernel(EstepArgs a, MfmaConst c) {
    estep_mfma_body<NT, NR, MODE, TU, V16>(a, c);
}
// The two-pass V16 soft sweep.  WPE: the waves per SIMD the register allocation is asked to reach.
template <int NR, bool REC>
__global__ __launch_bounds__(128) void estep_twopass_kernel(EstepArgs a, MfmaConst c) {
    estep_mfma_body<4, NR, SBCE_ESTEP_SOFT, 4, true, true, REC>(a, c);
}
bool make_mfma(const Problem& pb, MfmaConst& c, size_t& lds, long& blocks) {
    HypSplit h;
    if (!hyp_split(pb, h) || h.JA < 16 || h.JB < 16) return false;    // (n_tx = 1: JA = 1)
    const long JA = h.JA, JB = h.JB;
    c.B = pb.B; c.Td = pb.Td; c.P = pb.P; c.M = pb.M; c.lm = h.lm;
    c.JA = (int)JA; c.JB = (int)JB;
    c.chunk = (int)(JA < kChunk ? JA : kChunk);
    const int NO = pb.NT * pb.NR;
    c.nparts = NO <= 64 ? 64 / NO : 1;
    const int steps = (2 * pb.NR + 3) / 4;
    c.nkt_pad = (int)((JB / 16 + 1) / 2 * 2);

    c.prune = !g_debug.estep_noprune;
    c.count = g_debug.estep_count;
    c.inv_s2 = 1.0 / (pb.varn * pb.varn);
    c.thr_d = kSkipThr * pb.varn * pb.varn;
    c.reg = 0.1 * pb.varn * pb.varn;
    // NT = 4: + the row-tile bound vectors P y, P h_0, P h_2 (P = projector onto
    // span(h_1, h_3)^perp), 3 NR complex
    c.rowb_off = 4 + 2 * NO + c.nkt_pad;
    c.prep_stride = c.rowb_off + (pb.NT == 4 ? 6 * pb.NR : 0);
    c.rec_words = c.prep_stride + 2 * pb.NR;
    c.tab_d = mfma_tab_d(NO, c.chunk, steps, pb.M, c.nkt_pad, c.rec_words);
    c.spw = 4;                                           // symbols per wave
    c.screen = !g_debug.estep_nof32;                     // FP32 tile-group screen (V16)
    c.tri = g_debug.estep_tri;                           // per-group bounds (V16)
    c.order = !g_debug.estep_noorder;                    // best-first order (V16, soft)
    c.twopass = !g_debug.estep_notwopass;                // two-pass V16 soft sweep
    c.rowb = pb.NT == 4 && c.prune;
    lds = 64 * sizeof(cd) + (size_t)kMfmaWaves * c.tab_d * sizeof(double);
    const long nsym = (long)pb.B * pb.Td;
    const long per_block = (long)kMfmaWaves * c.spw;
    blocks = (nsym + per_block - 1) / per_block;
    return lds <= 160 * 1024;
}

template <int NT, int NR>
hipError_t dispatch_mfma_mode(const MfmaConst& c, size_t lds, long blocks, const EstepArgs& a,
                              int mode, hipStream_t s) {
    const bool tu4 = (c.chunk / 16) % 4 == 0;
    if constexpr (NT == 4) {                      // the V16 body exists for n_tx = 4 alone
        if (c.M == 16 && tu4) {                   // cfg1 geometry: hoisted V operand
            // the V16 body takes these layout constants as compile-time values
            if (c.JA != 256 || c.JB != 256 || c.chunk != 256 || c.nkt_pad != 16 ||
                c.prep_stride != 4 + 2 * NT * NR + 16 + 6 * NR)
                return hipErrorInvalidValue;
            if (mode == SBCE_ESTEP_HARD) {
                hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_HARD, 4, true>),
                                   dim3((unsigned)blocks), dim3(64 * kMfmaWaves), lds, s, a, c);
                return hipGetLastError();
            }
            if constexpr (SBCE_AB) {              // the product build has no one-pass soft instance
                if (!c.twopass) {
                    hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_SOFT, 4, true>),
                                       dim3((unsigned)blocks), dim3(64 * kMfmaWaves), lds, s, a, c);
                    return hipGetLastError();
                }
            }
            // two-pass: the record's second half only where a wave sweeps symbols in series
            const size_t lds2 = a.list ? lds - kMfmaWaves * mfma_rec_half_v16(NT, NR) * sizeof(double) : lds;
            if (a.prep)
                hipLaunchKernelGGL((estep_twopass_kernel<NR, true>), dim3((unsigned)blocks),
                                   dim3(64 * kMfmaWaves), lds2, s, a, c);
            else
                hipLaunchKernelGGL((estep_twopass_kernel<NR, false>), dim3((unsigned)blocks),
                                   dim3(64 * kMfmaWaves), lds2, s, a, c);
            return hipGetLastError();
        }
    }
    if (mode == SBCE_ESTEP_HARD) {
        if (tu4)
            hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_HARD, 4>), dim3((unsigned)blocks),
                               dim3(64 * kMfmaWaves), lds, s, a, c);
        else
            hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_HARD, 1>), dim3((unsigned)blocks),
                               dim3(64 * kMfmaWaves), lds, s, a, c);
    } else {
        if (tu4)
            hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_SOFT, 4>), dim3((unsigned)blocks),
                               dim3(64 * kMfmaWaves), lds, s, a, c);
        else
            hipLaunchKernelGGL((estep_mfma_kernel<NT, NR, SBCE_ESTEP_SOFT, 1>), dim3((unsigned)blocks),
                               dim3(64 * kMfmaWaves), lds, s, a, c);
    }
    return hipGetLastError();
}

template <int NT>
hipError_t dispatch_mfma_nr(int NR, const MfmaConst& c, size_t lds, long blocks,
                            const EstepArgs& a, int mode, hipStream_t s) {
    switch (NR) {
        case 1: return dispatch_mfma_mode<NT, 1>(c, lds, blocks, a, mode, s);
        case 2: return dispatch_mfma_mode<NT, 2>(c, lds, blocks, a, mode, s);
        case 3: return dispatch_mfma_mode<NT, 3>(c, lds, blocks, a, mode, s);
        case 4: return dispatch_mfma_mode<NT, 4>(c, lds, blocks, a, mode, s);
        case 5: return dispatch_mfma_mode<NT, 5>(c, lds, blocks, a, mode, s);
        case 6: return dispatch_mfma_mode<NT, 6>(c, lds, blocks, a, mode, s);
        case 7: return dispatch_mfma_mode<NT, 7>(c, lds, blocks, a, mode, s);
        case 8: return dispatch_mfma_mode<NT, 8>(c, lds, blocks, a, mode, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t estep_debug_mfma(unsigned long long* out, int reset) {
    if (reset) {
        const unsigned long long z = 0;
        return hipMemcpyToSymbol(HIP_SYMBOL(g_estep_mfma), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_estep_mfma), sizeof(*out), 0,
                               hipMemcpyDeviceToHost);
}

hipError_t estep_debug_pass2(unsigned long long* out, int reset) {
    if (reset) {
        const unsigned long long z = 0;
        return hipMemcpyToSymbol(HIP_SYMBOL(g_estep_pass2), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_estep_pass2), sizeof(*out), 0,
                               hipMemcpyDeviceToHost);
}

hipError_t estep_debug_groups(unsigned long long* out, int reset) {
    if (reset) {
        const unsigned long long z = 0;
        return hipMemcpyToSymbol(HIP_SYMBOL(g_estep_groups), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_estep_groups), sizeof(*out), 0,
                               hipMemcpyDeviceToHost);
}

SweepPlan estep_sweep_plan(const Problem& pb) {
    MfmaConst c;
    size_t lds;
    long blocks;
    if (!make_mfma(pb, c, lds, blocks)) return SweepPlan{};
    return SweepPlan{true, c.lm, c.JB, c.prep_stride, c.count, c.reg, c.inv_s2, c.thr_d, blocks};
}

int estep_prep_stride(const Problem& pb) { return estep_sweep_plan(pb).prep_stride; }

// blocks: the plan's, or fewer for a listed sweep (the waves grab symbols off EstepArgs::list)
hipError_t launch_estep_sweep(const Problem& pb, const EstepArgs& a, int mode, long blocks,
                              hipStream_t s) {
    MfmaConst c;
    size_t lds;
    long all;
    if (!make_mfma(pb, c, lds, all)) return hipErrorInvalidValue;
    switch (pb.NT) {
        case 2: return dispatch_mfma_nr<2>(pb.NR, c, lds, blocks, a, mode, s);
        case 3: return dispatch_mfma_nr<3>(pb.NR, c, lds, blocks, a, mode, s);
        case 4: return dispatch_mfma_nr<4>(pb.NR, c, lds, blocks, a, mode, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sbce
