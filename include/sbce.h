/*
 * sbce.h — C-ABI of libsbce.so, the MI355X-native EM semi-blind channel
 * estimator for the MIMO-RIS cascaded channel.
 *
 * Drop-in boundary.  The reference has no native code: its
 * operator is the Python function
 *     em(Y_d, Y_p, T_d, T_p, Z_p, PsiTilde_td, all_possibleSymbols, M, varn,
 *        itera, h_initial) -> theta (K,1) complex128
 * ("Proposed method/Proposed_method_NMSEvsTp.py":50-83, called at :165; same
 * contract at "Proposed method/Proposed_method_NMSEvsTd.py":44/150 and
 * "Proposed method/SNR/all_Detectors.py":242/377).  The build's Python shim
 * (package em.py) keeps that signature, stacks the per-symbol lists into
 * batch-major device buffers and calls sbce_em() through ctypes.  Every entry
 * point below is what that ctypes binding declares.
 *
 * Conventions
 *   - complex numbers are interleaved float64 pairs (re, im), i.e. numpy
 *     complex128 / torch.complex128 memory;
 *   - every pointer in sbce_ptrs is a DEVICE pointer owned by the caller
 *     (e.g. torch.empty(..., device="cuda").data_ptr()); the library never
 *     allocates, keeps no global state and never synchronises the stream;
 *   - all work is stream-ordered on `hip_stream` (a hipStream_t, 0 = default);
 *   - return value 0 on success, a negative SBCE_E* code otherwise; nothing
 *     throws across the ABI.  Per-trial numerical status goes to ptrs->status.
 *
 * Batch-major layouts (B = dims.batch, P = dims.n_psi = N+1 with the direct
 * path, L = P*n_tx, K = L*n_rx):
 *   y_d      [B][T_d][n_rx]          data observations   (reference Y_d list)
 *   y_p      [B][T_p][n_rx]          pilot observations  (reference Y_p list)
 *   psi_d    [B][T_d][P]             RIS phases, TRANSPOSED reference
 *                                    PsiTilde_td ((N+1) x T_d, row 0 = direct)
 *   u_p      [B][T_p][L]             pilot regressors u_p = psi_p (x) x_p, i.e.
 *                                    Z_p[t] = u_p^T (x) I_{n_rx}
 *   cons     [M]                     constellation, table order of
 *                                    all_possibleSymbols' last column
 *   theta    [B][K]                  in: h_initial, out: estimate; reference
 *                                    vec order theta[(p*n_tx+a)*n_rx + r]
 *   x_d_true [B][T_d][n_tx]          optional (LLF genie term)
 *   llf      [B][iters] float64      optional output (IterationsvsLLF.py:76)
 *   h_true   [B][K]                  optional: enables the reference's oracle
 *                                    early stop (PM.py:110-112)
 *   iters_done [B] int32             optional output: iterations performed
 *   status   [B] int32               per-trial flags (SBCE_STATUS_*)
 *   x_dest   [B][T_d][n_tx]          optional output: last-iteration decisions
 *   x_sup    [B][T_d][n_tx]          optional superimposed pilot symbols
 *   varn_t   [B] float64             optional per-trial noise variances (ABI 6)
 */
#ifndef SBCE_H_
#define SBCE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBCE_ABI_VERSION 7

/* return codes */
#define SBCE_OK 0
#define SBCE_EINVAL (-1)        /* bad dims / null pointer / misaligned */
#define SBCE_EUNSUPPORTED (-2)  /* shape outside the compiled kernel set */
#define SBCE_EHIP (-3)          /* a HIP launch failed */
#define SBCE_EWORKSPACE (-4)    /* workspace too small */

/* E-step modes */
#define SBCE_ESTEP_SOFT 0       /* exact posterior over all M^n_tx hypotheses:
                                   Proposed_method_NMSEvsTp.py:61-71 */
#define SBCE_ESTEP_HARD 1       /* argmax posterior ("log-max"):
                                   ML_detecctor.py:65-77 */
#define SBCE_ESTEP_PM 2         /* partitioned list detector, every list member
                                   weight 1: PM.py:57-104 (dims.partition_r) */
#define SBCE_ESTEP_PM_SOFT 3    /* partitioned list detector, posterior list
                                   weights: PM_beta.py:55-95 (dims.partition_r) */
#define SBCE_ESTEP_ZF 4         /* zero-forcing hard decision (n_rx >= n_tx):
                                   all_detectorsvsTd.py:98-133 */
#define SBCE_ESTEP_MMSE 5       /* MMSE hard decision: all_detectorsvsTd.py:54-96 */
#define SBCE_ESTEP_GAUSS 6      /* Gaussian-prior EM (x ~ CN(0, varx^2 I), no constellation):
                                   MIMO_Gaussian_proposed.py:56-89.  m_t = LMMSE mean, S_t = the
                                   posterior covariance WITHOUT m m^H (the reference adds the
                                   scalar ||mu_t||^2 to every entry instead, :73-75; for n_rx = 1
                                   that term is kept as R += c 1 1^T, for n_rx >= 2 it cancels
                                   in the pseudo-inverse, see sbce_gauss_expand).  P = N rows of
                                   psi (no direct path); dims.varx used; cons ignored */
#define SBCE_ESTEP_MMSE_SOFT 7  /* soft MMSE E-step for n_tx = 1..8: see SBCE_ESTEP_ZF_SOFT */
#define SBCE_ESTEP_ZF_SOFT 8    /* soft ZF E-step.  Both soft modes (an additive extension of
                                   ABI 7): per-stream linear equalisation and a Gaussian soft
                                   demapper, O(n_tx^3 + n_tx M) per symbol -- the arithmetic of
                                   sbce_detect_linear (below) inside the EM chain.  Per (b, t) on the
                                   CLEAN effective channel H_t[r][a] = sum_p psi_d[b][t][p]
                                   theta[b][(p n_tx + a) n_rx + r] (not the reference's off-by-one
                                   channel of SBCE_ESTEP_ZF / _MMSE), with s2 = varn_b^2 (varn_t[b]
                                   or dims.varn: the posterior denominator of every E-step here),
                                   es = (sum_s |cons[s]|^2) / M (formed on the device from the
                                   table), rho = s2 / es (MMSE) or 0 (ZF) and A = H^H H + rho I by
                                   Cholesky: g, z, mu, x_soft and nu as documented for
                                   sbce_detect_linear; post[a][s] ~ e^{-|x_soft_a - cons[s]|^2 / nu_a},
                                   m_a = sum_s post cons, S[a][a] = sum_s post |cons|^2 and
                                   S[a][c] = m_a conj(m_c) for a != c (a product posterior, so
                                   S - m m^H = diag(var) >= 0 in sbce_em_noise).
                                   Degenerate cases: a pivot <= 1e-14 max_a A_aa gives the whole
                                   symbol the uniform posterior's moments and sets
                                   SBCE_STATUS_DETECTOR; an MMSE stream with mu_a <= 0 gets the
                                   uniform posterior for itself alone.  Every output is finite for
                                   any s2 > 0.
                                   Limits (decided before any HIP call): n_tx 1..8, n_rx 1..8, m a
                                   power of two in 2..64, and n_rx >= n_tx for ZF_SOFT, else
                                   SBCE_EUNSUPPORTED (also for n_tx or n_rx past 8); x_dest or x_sup
                                   set: SBCE_EINVAL (no hard decisions, no superimposed pilots);
                                   partition_r and varx are ignored.  Accepted by sbce_estep,
                                   sbce_em, sbce_em_multi (the fixed-point rule applies as for any
                                   mode), sbce_em_noise and sbce_em_conv (the theta rule at every
                                   n_tx; ll_hist keeps sbce_loglik's own n_tx <= 4 limit).
                                   Deterministic: trial b of a B-trial call is bitwise the B = 1
                                   call, varn_t[b] == dims.varn gives the scalar call's bits */
/* value 9 is not a mode (SBCE_EUNSUPPORTED) */
#define SBCE_ESTEP_EP 10        /* expectation-propagation E-step for n_tx = 1..8 (an additive
                                   extension of ABI 7; Cespedes et al., "Expectation Propagation
                                   Detection for High-Order High-Dimensional MIMO Systems", IEEE
                                   Trans. Commun. 2014): p passes of the MMSE_SOFT solve, each with
                                   the per-stream posterior means and variances of the pass before
                                   as a Gaussian prior.  Per (b, t), with H, s2 and es as for
                                   MMSE_SOFT, G = H^H H, u = H^H y and per stream a the state r_a
                                   (real), q_a (complex), starting at r_a = s2 / es, q_a = 0; pass
                                   l = 1..p:
                                     A = G + diag(r) by Cholesky (same pivot rule);
                                     g_a = (A^-1)_aa, z = A^-1 (u + q);
                                     mu_a = 1 - r_a g_a, h2_a = s2 g_a / mu_a (cavity variance),
                                     t_a = (z_a - g_a q_a) / mu_a (cavity mean);
                                     post[a][s] ~ e^{-|t_a - cons[s]|^2 / h2_a},
                                     m_a = sum_s post cons, s_a = sum_s post |cons|^2;
                                     unless l = p: v_a = max(s_a - |m_a|^2, 5e-7 es),
                                     r' = s2 (1/v_a - 1/h2_a), q' = s2 (m_a/v_a - t_a/h2_a) and, when
                                     r' is finite and > 0, r_a <- (r' + r_a) / 2, q_a <- (q' + q_a) / 2
                                     (damping 0.5; otherwise both keep their values).
                                   Pass 1 is MMSE_SOFT.  Moments of the last pass in MMSE_SOFT's
                                   product form: m_a, S[a][a] = s_a, S[a][c] = m_a conj(m_c).
                                   dims.partition_r carries p: 0 gives the default 5, 1..16 are
                                   taken as given, above 16: SBCE_EINVAL.
                                   Degenerate cases: a failed pivot in any pass gives the whole
                                   symbol the uniform posterior's moments and sets
                                   SBCE_STATUS_DETECTOR; a stream with mu_a <= 0 in a pass gets the
                                   uniform posterior for itself in that pass and keeps its r and q.
                                   Every output is finite for any s2 > 0.
                                   Limits, errors, entry points and determinism are MMSE_SOFT's
                                   (n_tx, n_rx 1..8, m a power of two in 2..64, else
                                   SBCE_EUNSUPPORTED; x_dest or x_sup: SBCE_EINVAL); every sum's
                                   order is fixed by (n_tx, n_rx, n_psi, m, p) */

/* M-step solve modes (SURVEY.md §7 hard part 3) */
#define SBCE_SOLVE_CHOL 0       /* Hermitian Cholesky of the reduced L x L system
                                   (== LU of the K x K reference system,
                                   Proposed_method_NMSEvsTp.py:80, on HPD R).  A pivot
                                   <= 1e-14 max diag R (R not numerically HPD: rank-deficient
                                   when T_p + n_tx T_d < L) sets SBCE_STATUS_NONHPD and its
                                   direction is dropped: theta stays finite, solves the normal
                                   equations, and its range-space part is lstsq's minimum-norm
                                   solution (the reference's LU returns rounding noise there) */
#define SBCE_SOLVE_CHOL_DROP 1  /* the same solve (kept for ABI 1-6 callers): non-HPD pivots
                                   dropped, a basic solution on the kept coordinates, NOT
                                   minimum-norm */
#define SBCE_SOLVE_MINNORM 2    /* minimum-norm least squares, np.linalg.lstsq of PM.py:108
                                   (the intended fallback of all_detectorsvsTd.py:238-241):
                                   R's rank is cut at eps*K*lambda_max(R) (lstsq's default
                                   rcond = eps*max(K,K) on the K x K system, whose singular
                                   values are R's eigenvalues), lambda_max by 4 Lanczos steps;
                                   R = G G^H by a Cholesky that drops the pivots below 32x the
                                   cut (above its rounding noise), theta = conj(G (G^H G)^-2
                                   G^H B^H).  Equal to lstsq when no pivot lies between 4x the
                                   cut and 2048x it (else SBCE_STATUS_RANK) and no eigenvalue
                                   of R lies just below the cut */

/* per-trial status bits */
#define SBCE_STATUS_NONHPD 1
#define SBCE_STATUS_PILOT 2     /* n_tx in {4, 8}: u_p is not a Kronecker product
                                   psi_p (x) x_p (PM.py:119-130), so the MFMA build's
                                   factored pilot term does not apply; R of the trial is
                                   rebuilt by the general (VALU) path (informational) */
#define SBCE_STATUS_DETECTOR 4  /* ZF/MMSE: the reference's flattened argmin indexed past
                                   all_possibleSymbols (IndexError at
                                   all_detectorsvsTd.py:52); row flat mod M^n_tx used.
                                   ZF_SOFT / MMSE_SOFT / EP: a symbol's A = H^H H + rho I (EP:
                                   G + diag(r) of some pass) had a pivot
                                   <= 1e-14 max_a A_aa; that symbol carries the uniform
                                   posterior's moments (NONHPD stays the M-step's finding about R
                                   in the chain's status word) */
#define SBCE_STATUS_DEBUG 8     /* a diagnostic phase-skip mask (sbce_debug_chol_skip, not
                                   part of this header's API) or a non-default kernel selected
                                   by an SBCE_* debug environment variable was active */
#define SBCE_STATUS_RANK 16     /* SBCE_SOLVE_MINNORM: a Cholesky pivot lay between 4x lstsq's
                                   rank cut and 2048x it, where the pivot-based rank may differ
                                   from the singular-value rank np.linalg.lstsq uses */
#define SBCE_STATUS_SINGULAR 32 /* sbce_approx_em: a pivot of the N x N normal matrix A was
                                   <= 1e-14 max_i |A_ii| (A singular: T_p + T_d < N); the trial
                                   stopped there and g holds its last finite iterate */

typedef struct sbce_dims {
    int32_t batch;      /* B: independent Monte-Carlo trials */
    int32_t n_tx;       /* streams (1..4 exact/hard E-step, 1..8 PM/ZF/MMSE and soft ZF/MMSE) */
    int32_t n_rx;       /* receive antennas (1..8) */
    int32_t n_psi;      /* P = rows of PsiTilde_td (N+1 with the direct path) */
    int32_t t_p;        /* pilot symbols */
    int32_t t_d;        /* data symbols */
    int32_t m;          /* constellation size (power of two, 2..64) */
    int32_t partition_r;/* PM modes: list = M^(p+1) with p = int(partition_r /
                           log2 M) (PM.py:74), at most 64 members; SBCE_ESTEP_EP: the pass
                           count (0 = 5, 1..16); else 0 */
    double varn;        /* noise variance parameter; posterior uses varn^2 */
    double varx;        /* SBCE_ESTEP_GAUSS only: symbol variance parameter, the prior
                           covariance uses varx^2 (MIMO_Gaussian_proposed.py:44); else ignored */
} sbce_dims;

typedef struct sbce_ptrs {
    const void* y_d;
    const void* y_p;
    const void* psi_d;
    const void* u_p;
    const void* cons;
    void* theta;
    const void* x_d_true;   /* may be NULL */
    double* llf;            /* may be NULL (requires x_d_true) */
    const void* h_true;     /* may be NULL */
    int32_t* iters_done;    /* may be NULL */
    int32_t* status;        /* may be NULL */
    void* workspace;
    size_t workspace_bytes;
    void* x_dest;           /* may be NULL; hard E-step modes only (HARD/ZF/MMSE):
                               [B][T_d][n_tx] decisions of the last E-step
                               (SER/log_max_SER.py:77-78) */
    const void* x_sup;      /* may be NULL; SOFT/HARD only: [B][T_d][n_tx] pilot
                               symbols superimposed on the data, hypotheses x_j + x_sup[t]
                               (Parallel/ParallelProtocol_Tp.py:63-86; t_p is then 0) */
    const double* varn_t;   /* may be NULL (ABI 6): [B] noise variance parameter of each trial,
                               used instead of dims.varn (which must still be > 0) by the E-step
                               posterior (varn^2) and the LLF.  Lets one call carry the trials of
                               several SNR points of a sweep (all_detectorsvsTd.py's grid, SNR/
                               all_Detectors.py:351-354): every trial's result is the one a call
                               with dims.varn = varn_t[b] gives.  8-byte aligned, values > 0 */
} sbce_ptrs;

/* ABI version (SBCE_ABI_VERSION). */
int sbce_abi_version(void);

/* Static description of an error code. */
const char* sbce_strerror(int code);

/* Device workspace needed by sbce_em / sbce_estep / sbce_mstep for `d` (every solve mode).
 * The size depends on the library version: re-query it after upgrading the library. */
int sbce_workspace_bytes(const sbce_dims* d, size_t* bytes);

/* Device workspace for `d` with ONE solve mode (SBCE_SOLVE_*): the min-norm Gram matrix
 * ([B][L][L] complex) and the tiled factorisation's tile inverses are only carved when that solve
 * needs them, so a SBCE_SOLVE_CHOL workspace at L <= 512 is about half the size.  sbce_em /
 * sbce_mstep accept any workspace at least this large for their solve_mode (ABI 5). */
int sbce_workspace_bytes_solve(const sbce_dims* d, int solve_mode, size_t* bytes);

/* Full EM: `iters` iterations of E-step + M-step on every trial of the batch.
 * Replaces em() at Proposed_method_NMSEvsTp.py:50-83 (estep_mode SOFT) and the
 * hard-ML em() at ML_detecctor.py:51-86 (estep_mode HARD, llf != NULL).
 * The chain is a deterministic function of theta per trial, so once an M-step returns the theta
 * it was given bit for bit, the trial's later iterations are not executed: they would reproduce
 * it.  theta, status, x_dest and iters_done (= iters) are those of the full chain, bit for bit;
 * only the time differs (high-SNR soft EM and hard-decision EM typically settle within a few
 * iterations).  This applies to the batched Cholesky solve (n_tx in {4, 8} or L > 64, L <= 512,
 * not SBCE_SOLVE_MINNORM) without h_true, llf and x_sup; every other call executes all
 * iterations, as do sbce_em_noise and sbce_em_conv (whose own rule stops trials). */
int sbce_em(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode,
            int solve_mode, void* hip_stream);

/* sbce_em on n = 1..8 independent problems at once (the stream sub-batches of one batch, or
 * unrelated calls), problem j on hip_streams[j], issued iteration by iteration over all of them --
 * and no longer than needed: where sbce_em's fixed-point rule applies (above) and the stream is
 * not being captured, the launch sequence of a problem ENDS once every one of its trials has
 * reached its fixed point.  The back substitution that freezes a problem's last live trial stores
 * a per-call generation number to a word of host-mapped memory; before issuing iteration
 * it >= lead the call waits for the event it recorded after iteration it - lead and reads the
 * word.  Every iteration after that point would touch nothing, so theta, status, x_dest and
 * iters_done (= iters) are bit for bit those of sbce_em; `lead` - 1 empty iterations are issued
 * instead of all the remaining ones.
 *   lead            1..iters: iterations the host may run ahead of the device; 0: the library's
 *                   default (2, or iters when smaller).
 *   iters_issued    host array [n] or NULL: iterations enqueued per problem (iters wherever the
 *                   rule does not apply, the stream is capturing or no end was seen).
 * Every stream of hip_streams must belong to the calling thread's CURRENT device (hipSetDevice):
 * the events and the counter of a paced problem are made on that device.
 * The call returns when everything is enqueued and does not synchronise at its end; outputs are
 * stream-ordered as sbce_em's.  UNLIKE sbce_em IT MAY BLOCK THE CALLING THREAD for up to the
 * duration of the run: it waits for events of its own, already enqueued launches (never for the
 * word itself, so never longer than the device works).  The pinned word, the device counter and
 * the events come from a small pool the library owns; a steady-state call allocates nothing.
 * Every argument of every problem is checked as sbce_em checks it before any HIP call: on
 * SBCE_EINVAL / SBCE_EUNSUPPORTED / SBCE_EWORKSPACE nothing was issued for any problem.
 * SBCE_EINVAL also: n outside 1..8, a null array, lead < 0 or lead > iters. */
int sbce_em_multi(int n, const sbce_dims* const* dims, const sbce_ptrs* const* ptrs, int iters,
                  int estep_mode, int solve_mode, void* const* hip_streams, int lead,
                  int* iters_issued);

/* One E-step: theta -> per-symbol posterior moments, written to `moments`
 * [B][T_d][n_tx + n_tx*n_tx] complex (m_t, then S_t row-major,
 * S_t[a][b] = E[x_a conj(x_b)]).  Test/diagnostic entry point for the
 * E-step of Proposed_method_NMSEvsTp.py:61-69. */
int sbce_estep(const sbce_dims* d, const sbce_ptrs* p, int estep_mode,
               void* moments, void* hip_stream);

/* One M-step from given moments: builds R = sum_p u u^H + sum_t (psi psi^H)(x)S_t
 * and B^H, solves R X = B^H and writes theta = conj(X) in reference vec order
 * (Proposed_method_NMSEvsTp.py:70-80 with commutation_matrix.py:3-8 applied).
 * If `r_out` / `rhs_out` are non-NULL the normal equations ([B][L][L] and
 * [B][L][n_rx] complex) are copied there before the solve. */
int sbce_mstep(const sbce_dims* d, const sbce_ptrs* p, const void* moments,
               int solve_mode, void* r_out, void* rhs_out, void* hip_stream);

/* Per-trial symbol error rates of decisions x_dest against x_d_true ([B][T_d][n_tx]):
 * ser_out[2b] = the SER expression of SER/log_max_SER.py:162 (count_nonzero of the
 * (T_d,n_tx,1) - (T_d,1,n_tx) broadcast, / (T_d n_tx)); ser_out[2b+1] = element-wise SER. */
int sbce_ser(const sbce_dims* d, const void* x_dest, const void* x_d_true, double* ser_out,
             void* hip_stream);

/* Gaussian-prior EM output in the reference's format: the n_rx x (N n_tx n_rx^2) matrix
 * H_l = B pinv(A) of MIMO_Gaussian_proposed.py:77-85, from the reduced estimate theta
 * ([B][K], K = N n_tx n_rx, the M-step of sbce_em with SBCE_ESTEP_GAUSS).  With
 * e = vec(I_{n_rx}), f = 1 - e, Lr = N n_tx and theta_r = row r of the reduced channel,
 *   n_rx >= 2:  H_l[r] = kron(theta_r, e^T) / n_rx - (theta_r . 1) / (Lr (n_rx^2 - n_rx)) kron(1, f^T)
 *   n_rx == 1:  H_l = theta^T
 * (the all-ones term c J the reference adds to A has range outside span kron(., e) for
 * n_rx >= 2, where c drops out of pinv(A)).  h_out: [B][n_rx][N n_tx n_rx^2] complex. */
int sbce_gauss_expand(const sbce_dims* d, const void* theta, void* h_out, void* hip_stream);

/* Per-trial NMSE ||theta - h||^2 / ||h||^2 (Proposed_method_NMSEvsTp.py:172). */
int sbce_nmse(const sbce_dims* d, const void* theta, const void* h_true,
              double* nmse_out, void* hip_stream);

/* ---- Semi-blind Gaussian-approximation EM (ABI 7): the comparator EM_approx of
 * "Comparision/Comparision T_d vs NMSE.py":106-145 (the same function at "Comparision/
 * Comparision T_p .py":74-113).  Model y_t = G^H psi_t x_t + z_t with G n_ris x n_rx, scalar
 * symbols (n_tx = 1), no direct path.  sbce_dims / sbce_ptrs are not used by these two entry
 * points.  Batch-major layouts, complex128:
 *   y_d   [B][T_d][n_rx]   reference Y_d (n_rx x L_d), transposed
 *   y_p   [B][T_p][n_rx]   reference Y_p (n_rx x L_p), transposed
 *   psi_d [B][T_d][n_ris]  reference PsiTilde_td (N x L_d), transposed
 *   psi_p [B][T_p][n_ris]  reference PsiTilde_tp (N x L_p), transposed
 *   x_p   [B][T_p]         pilot symbols
 *   g     [B][n_ris][n_rx] in: G_0 = conj(Y_p pinv(Psi_p diag(x_p)))^T (:107-108, computed by
 *                          the caller); out: the estimate after `iters` updates */
typedef struct sbce_approx_dims {
    int32_t batch;      /* B: independent trials */
    int32_t n_ris;      /* N: RIS elements (1..64) */
    int32_t n_rx;       /* M: receive antennas (1..8) */
    int32_t t_p;        /* pilot symbols (>= 1) */
    int32_t t_d;        /* data symbols (>= 1) */
    int32_t reserved;   /* 0 */
    double varn;        /* noise variance parameter; the estimator uses varn^2 (:124, :128) */
} sbce_approx_dims;

typedef struct sbce_approx_ptrs {
    const void* y_d;
    const void* y_p;
    const void* psi_d;
    const void* psi_p;
    const void* x_p;
    void* g;
    const double* varn_t;   /* may be NULL: [B] per-trial varn, as sbce_ptrs.varn_t */
    int32_t* status;        /* may be NULL: [B] SBCE_STATUS_* (SBCE_STATUS_SINGULAR) */
    void* workspace;        /* may be NULL when sbce_approx_workspace_bytes reports 0 */
    size_t workspace_bytes;
} sbce_approx_ptrs;

/* Device workspace of sbce_approx_em for `d` (0 in this version: the state of a trial lives in
 * LDS and registers). */
int sbce_approx_workspace_bytes(const sbce_approx_dims* d, size_t* bytes);

/* `iters` updates of the Gaussian-approximation EM on every trial, in one kernel launch (the
 * reference's `while i <= Iterations` performs Iterations + 1 updates).  A trial whose normal
 * matrix is singular gets SBCE_STATUS_SINGULAR and keeps its last finite iterate; the call
 * still returns 0.  SBCE_EINVAL: null required pointer, varn <= 0, iters < 1, batch < 1,
 * t_p < 1, t_d < 1; SBCE_EUNSUPPORTED: n_ris > 64 or n_rx > 8 (checked before any HIP call). */
int sbce_approx_em(const sbce_approx_dims* d, const sbce_approx_ptrs* p, int iters,
                   void* hip_stream);

/* ---- Batched data detector and soft demapper (an additive extension of ABI 7: no existing
 * struct or entry point changes, so the version number stays): decisions, symbol posteriors and bit
 * L-values of every data symbol of a batch from a GIVEN channel estimate theta (any estimator's
 * output, the pilot-only start, or the true channel).  Per (trial b, data symbol t) the effective
 * channel is H_t[r][a] = sum_p psi_d[b][t][p] theta[b][(p n_tx + a) n_rx + r] (the E-step's
 * layout); over the J = M^n_tx hypotheses x_j in itertools.product order (first stream slowest)
 * with d_j = ||y_t - H_t x_j||^2 and s2 the posterior denominator:
 *   x_hat, idx_hat  joint decision argmin_j d_j, ties to the lowest j (np.argmin)
 *   post[a][s]      sum_{j: x_j[a] = cons[s]} e^{-d_j/s2} / sum_j e^{-d_j/s2}
 *   llr[a][i]       log sum_{bit_i = 0} e^{-d_j/s2} - log sum_{bit_i = 1} e^{-d_j/s2}, with
 *                   bit_i(s) = (labels[s] >> i) & 1, i < log2 M: the L-value log(p0 / p1) of
 *                   "Proposed method/QAM.py":164-185 (bits LSB-first, :8-11) on the MIMO
 *                   posterior; with SBCE_DETECT_MAXLOG (min_{bit_i = 1} d_j - min_{bit_i = 0} d_j) / s2
 *   err[b]          {symbol entries with idx_hat != the table index nearest x_d_true, differing
 *                   label bits} of trial b (integer adds)
 * All sums are formed in the log domain (per-class minimum shifts), so every output is finite
 * for any s2 > 0.  cons is ANY table of M complex points and labels any permutation of 0..M-1:
 * no grid structure is assumed.  Results of a trial do not depend on the batch around it.
 * sbce_dims / sbce_ptrs are not used.  Batch-major layouts (complex128 unless noted):
 *   y_d      [B][T_d][n_rx]            psi_d  [B][T_d][P]       cons  [M]      theta [B][K]
 *   labels   [M] int32                 sigma2_t [B] float64     x_d_true [B][T_d][n_tx]
 *   x_hat    [B][T_d][n_tx]            idx_hat [B][T_d][n_tx] int32
 *   post     [B][T_d][n_tx][M] float64 llr    [B][T_d][n_tx][log2 M] float64
 *   err      [B][2] int32 */
#define SBCE_DETECT_MAXLOG 1    /* sbce_detect_dims.flags bit 0: max-log L-values in `llr` */

typedef struct sbce_detect_dims {
    int32_t batch;      /* B: independent trials (>= 1) */
    int32_t n_tx;       /* streams (1..4) */
    int32_t n_rx;       /* receive antennas (1..8) */
    int32_t n_psi;      /* P = rows of PsiTilde_td (>= 1) */
    int32_t t_d;        /* data symbols (>= 1) */
    int32_t m;          /* table size (power of two, 2..64), J = m^n_tx <= 65536 */
    int32_t flags;      /* SBCE_DETECT_*; every other bit 0 */
    double sigma2;      /* the posterior denominator itself (> 0): varn^2 for the EM posterior
                           (Proposed_method_NMSEvsTp.py:66), varn for the noise the data carry */
} sbce_detect_dims;

typedef struct sbce_detect_ptrs {
    const void* y_d;
    const void* psi_d;
    const void* cons;
    const void* theta;
    const int32_t* labels;   /* may be NULL unless llr or err is set */
    const double* sigma2_t;  /* may be NULL: [B] per-trial sigma2 (values > 0), as sbce_ptrs.varn_t */
    const void* x_d_true;    /* may be NULL unless err is set */
    void* x_hat;             /* may be NULL */
    int32_t* idx_hat;        /* may be NULL */
    double* post;            /* may be NULL */
    double* llr;             /* may be NULL (requires labels) */
    int32_t* err;            /* may be NULL (requires x_d_true and labels); zeroed by the call */
    void* workspace;         /* may be NULL when sbce_detect_workspace_bytes reports 0 */
    size_t workspace_bytes;
} sbce_detect_ptrs;

/* Device workspace of sbce_detect for `d` (0 in this version: a symbol's state lives in LDS and
 * registers). */
int sbce_detect_workspace_bytes(const sbce_detect_dims* d, size_t* bytes);

/* One detection pass over every (trial, data symbol): one memset of `err` (when set) and one
 * kernel launch on `hip_stream`, no allocation, no synchronisation; capturable in a HIP graph.
 * Decided before any HIP call -- SBCE_EINVAL: null dims / ptrs / required pointer, batch, t_d,
 * n_psi, n_tx or n_rx < 1, m not a power of two in 2..64, sigma2 <= 0, llr without labels, err
 * without x_d_true or labels, unknown flag bits, a misaligned pointer (16 bytes complex, 8 float64,
 * 4 int32); SBCE_EUNSUPPORTED: n_tx > 4, n_rx > 8 or m^n_tx > 65536; SBCE_EWORKSPACE. */
int sbce_detect(const sbce_detect_dims* d, const sbce_detect_ptrs* p, void* hip_stream);

/* ---- EM with unknown noise variance (an additive extension of ABI 7: no existing struct or entry
 * point changes).  The noise parameter is estimated per trial beside theta: after an M-step, from
 * the new theta and the moments (m_t, S_t) of the same iteration's E-step,
 *   Q       = sum_pilots ||y_p - H_c u_p||^2 + sum_data ( ||y_t - H_t m_t||^2 + tr(H_t C_t H_t^H) )
 *   sigma^2 = Q / (n_rx (T_p + T_d)),      varn_est = sqrt(sigma^2)
 * with C_t = S_t - m_t m_t^H and H_t[r][a] = sum_p psi_d[t][p] theta[(p n_tx + a) n_rx + r]
 * (sbce_detect's channel, also in the PM modes).  The posterior of the next E-step divides by
 * varn_est^2 = sigma^2: this is the exact M-step for the denominator, so with SBCE_ESTEP_SOFT the
 * observed-data likelihood does not decrease.  Rules: sigma^2 < varn_min^2 gives varn_est =
 * varn_min exactly and SBCE_STATUS_NOISE; a non-finite Q keeps the previous value, same bit.
 * The sums are formed without atomics in an order fixed by (t_d, t_p, n_rx): a trial's result
 * does not depend on the batch around it. */
#define SBCE_STATUS_NOISE 64    /* the noise update hit its floor varn_min, or Q was not finite and
                                   the previous parameter was kept */

typedef struct sbce_noise_opts {
    double* varn_est;     /* [B] out: the parameter after the last update a trial performed */
    double* varn_hist;    /* may be NULL: [B][iters] out, the parameter after each iteration
                             (sbce_noise_var: ignored) */
    void* scratch;        /* device scratch, 8-byte aligned */
    size_t scratch_bytes; /* at least sbce_noise_workspace_bytes */
    double varn_min;      /* > 0: floor of the parameter */
    int32_t flags;        /* 0 */
} sbce_noise_opts;

/* Device scratch of sbce_noise_var / sbce_em_noise for `d` (the block sums of Q). */
int sbce_noise_workspace_bytes(const sbce_dims* d, size_t* bytes);

/* One noise update of every trial from theta (p->theta, not written) and `moments` (sbce_estep's
 * layout): two kernel launches on `hip_stream`, no memset, no allocation, no synchronisation;
 * capturable in a HIP graph as a linear chain.  The previous value of the keep-previous rule is
 * p->varn_t[b] (or d->varn); p->status, when set, is written (0 or SBCE_STATUS_NOISE).  p->cons
 * and p->workspace are not used.  Errors as sbce_em_noise. */
int sbce_noise_var(const sbce_dims* d, const sbce_ptrs* p, const void* moments,
                   const sbce_noise_opts* o, void* hip_stream);

/* sbce_em with the noise parameter estimated: varn_est[b] starts at p->varn_t[b] (or d->varn) and
 * is the E-step's per-trial parameter; per iteration E-step, M-step, noise update, then the oracle
 * early stop (p->h_true), so a trial's last M-step is followed by its update.  p->workspace as for
 * sbce_em.  estep_mode: SOFT, HARD, PM, PM_SOFT, ZF, MMSE, MMSE_SOFT, ZF_SOFT, EP; SBCE_ESTEP_GAUSS gives
 * SBCE_EUNSUPPORTED (its S_t is not a second moment).  Decided before any HIP call, beside
 * sbce_em's own checks -- SBCE_EINVAL: p->x_sup or p->llf set, null or misaligned (8 bytes)
 * varn_est, varn_hist or scratch, varn_min <= 0, flags != 0; SBCE_EWORKSPACE: scratch_bytes too
 * small. */
int sbce_em_noise(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode,
                  int solve_mode, const sbce_noise_opts* o, void* hip_stream);

/* ---- Observed-data log-likelihood and a truth-free convergence stop (an additive extension of
 * ABI 7: no existing struct or entry point changes).  The quantity the SOFT EM ascends, per trial
 * b with s2 = varn_b^2 (p->varn_t[b], or d->varn), J = M^n_tx and d_j = ||y_t - H_t x_j||^2 over
 * the hypotheses in itertools.product order, H_t being the channel of the detector above:
 *   ll_sym[b][t] = -d_min/s2 + log sum_j e^{-(d_j - d_min)/s2} - log J - n_rx log(pi s2)
 *   ll[b]        = sum_t ll_sym[b][t] + sum_pilots ( -||y_p - H_c u_p||^2/s2 - n_rx log(pi s2) )
 * (the pilot term is empty when t_p = 0).  The minimum-shifted sum has a term equal to 1, so
 * every output is finite for any s2 > 0.  No floating-point atomic is used and every reduction
 * order is fixed by the shape alone: a trial's bits do not depend on the batch around it. */

/* Device scratch of the log-likelihood call for `d`. */
int sbce_loglik_workspace_bytes(const sbce_dims* d, size_t* bytes);

/* ll [B] (and ll_sym [B][T_d] when not NULL) of every trial from p->theta, which is read and
 * never written: two kernel launches on `hip_stream`, no memset, no allocation, no
 * synchronisation; capturable in a HIP graph as a linear chain.  Uses p->y_d, y_p, psi_d, u_p,
 * cons, theta and varn_t; p->workspace, llf, h_true and status are not used.  Decided before any
 * HIP call -- SBCE_EINVAL: bad dims (varn <= 0 among them), a null or misaligned required
 * pointer (16 bytes complex, 8 bytes float64: ll, ll_sym, varn_t, scratch), p->x_sup set;
 * SBCE_EUNSUPPORTED: n_tx > 4, n_rx > 8, m not a power of two in 2..64 or m^n_tx > 65536 (the
 * detector's limits); SBCE_EWORKSPACE: scratch_bytes too small. */
int sbce_loglik(const sbce_dims* d, const sbce_ptrs* p, double* ll, double* ll_sym, void* scratch,
                size_t scratch_bytes, void* hip_stream);

#define SBCE_STATUS_CONVERGED 128   /* the trial stopped by a rule of sbce_conv_opts */

typedef struct sbce_conv_opts {
    double tol_theta;     /* >= 0: stop when ||theta_l - theta_{l-1}||^2 <= tol_theta^2 ||theta_l||^2
                             (theta_{-1} is the caller's h_initial; 0 stops at an exact fixed point) */
    double tol_ll;        /* >= 0; > 0 requires ll_hist: stop when l >= 1 and
                             ll_l - ll_{l-1} <= tol_ll |ll_l|; 0 switches the rule off */
    int32_t min_iters;    /* >= 1: no stop before this many iterations were performed */
    int32_t flags;        /* 0 */
    double* dtheta_hist;  /* may be NULL: [B][iters] sqrt(||dtheta||^2 / ||theta_l||^2) after each
                             iteration */
    double* ll_hist;      /* may be NULL: [B][iters] ll after each iteration (costs one log-likelihood
                             pass per iteration) */
    void* scratch;        /* device scratch, 16-byte aligned */
    size_t scratch_bytes; /* at least sbce_conv_workspace_bytes */
} sbce_conv_opts;

/* Device scratch of the convergence stop for `d`; want_ll != 0 when ll_hist is set. */
int sbce_conv_workspace_bytes(const sbce_dims* d, int want_ll, size_t* bytes);

/* The EM chain with a per-trial stop that needs no ground truth.  nz == NULL: the iterations of
 * sbce_em; nz set: those of sbce_em_noise.  Per iteration l: E-step, M-step, noise update (nz),
 * log-likelihood at the new theta and the current noise parameter (ll_hist), then one launch that
 * forms both norms in a fixed order, writes the histories and decides.  A trial that stops gets
 * SBCE_STATUS_CONVERGED and iters_done = l + 1 and is masked from then on exactly as an
 * oracle-stopped trial; its later history entries (varn_hist too) keep their last value.  The
 * decision has no division and a NaN never stops a trial.  While no trial can stop (min_iters =
 * iters) theta is bitwise the plain chain's.  Launches per iteration beside the chain's own: one,
 * or three with ll_hist.  Decided before any HIP call, beside the chain's own checks --
 * SBCE_EINVAL: cv NULL, p->h_true, p->llf or p->x_sup set (the point is to need no truth), a
 * negative or NaN tolerance, tol_ll > 0 without ll_hist, min_iters < 1, flags != 0, a misaligned
 * history (8 bytes) or a null or misaligned scratch (16 bytes); SBCE_EUNSUPPORTED:
 * SBCE_ESTEP_GAUSS, or ll_hist beyond the log-likelihood's limits; SBCE_EWORKSPACE.  The theta
 * rule works in every other E-step mode, PM at n_tx = 8 included. */
int sbce_em_conv(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
                 const sbce_noise_opts* nz, const sbce_conv_opts* cv, void* hip_stream);

/* ---- Linear soft detection (an additive extension of ABI 7: no existing struct or entry point
 * changes): per-stream ZF / LMMSE equalisation with a Gaussian soft demapper, for 1..8 streams,
 * from a GIVEN channel estimate theta.  Per (trial b, data symbol t) with H = H_t the effective
 * channel of the detector above, rho = sigma2 / es (MMSE) or 0 (ZF), A = H^H H + rho I (Hermitian
 * n_tx x n_tx, factored by Cholesky), g_a = (A^-1)_aa and z = A^-1 H^H y:
 *   MMSE  mu_a = 1 - rho g_a,  x_soft_a = z_a / mu_a,  nu_a = es (1 - mu_a) / mu_a
 *   ZF    x_soft_a = z_a,      nu_a = sigma2 g_a
 * x_soft is the unbiased estimate of stream a and nu its effective noise variance.  Each stream
 * is demapped on its own with d_s = |x_soft_a - cons[s]|^2:
 *   idx_hat[a]   argmin_s d_s, ties to the lowest s;  x_hat = cons[idx_hat]
 *   post[a][s]   e^{-d_s/nu_a} / sum_s e^{-d_s/nu_a}
 *   llr[a][i]    log sum_{bit_i = 0} e^{-d_s/nu_a} - log sum_{bit_i = 1} e^{-d_s/nu_a}, with
 *                bit_i(s) = (labels[s] >> i) & 1; with SBCE_DETECT_MAXLOG
 *                (min_{bit_i = 1} d_s - min_{bit_i = 0} d_s) / nu_a
 *   err[b]       the two integer counters of the detector above
 *   moments      m_a = sum_s post[a][s] cons[s], S[a][a] = sum_s post[a][s] |cons[s]|^2 and
 *                S[a][c] = m_a conj(m_c) for a != c, in the E-step's layout (m_t, then S_t)
 * Every sum is min-shifted in the log domain (its smallest member has weight 1), so every output
 * is finite for any sigma2 > 0, with one exception.  A Cholesky pivot <= 1e-14 max_a A_aa (the
 * pivot rule of SBCE_SOLVE_CHOL) makes the whole symbol carry no information: x_soft = 0 and
 * nu = +inf for every stream, so post = 1/M, llr = 0, idx_hat is the table point nearest 0
 * (lowest index on ties), the moments follow from the uniform post, and the trial gets
 * SBCE_STATUS_NONHPD; other symbols and trials are unaffected.  A single MMSE stream with
 * mu_a <= 0 (a zero channel column) is given the same outputs for that stream alone, and no
 * status bit: its matrix is sound.  Results of a trial do not depend on the batch around it.
 * Layouts as for the detector above, and
 *   x_soft [B][T_d][n_tx] complex    nu [B][T_d][n_tx] float64
 *   moments [B][T_d][n_tx + n_tx^2] complex    status [B] int32 */
#define SBCE_LINEAR_MMSE 0
#define SBCE_LINEAR_ZF 1
/* kind 2 is not a kind (SBCE_EINVAL) */
#define SBCE_LINEAR_EP 3        /* expectation propagation, the passes of SBCE_ESTEP_EP (above) with
                                   s2 = sigma2 and the caller's es (> 0): x_soft = t and nu = h2 of
                                   the last pass -- the extrinsic estimate of each stream and its
                                   variance -- and idx_hat, x_hat, post, llr, err and moments follow
                                   from them exactly as they follow from (x_soft, nu) of MMSE.  A
                                   failed pivot in any pass gives the symbol x_soft = 0, nu = +inf
                                   and the trial SBCE_STATUS_NONHPD; a stream with mu_a <= 0 in the
                                   last pass gets the same outputs for itself alone */
/* flags bits 8..15 of SBCE_LINEAR_EP: the pass count, 0 = the default 5, 1..16; above 16:
 * SBCE_EINVAL.  For the other kinds these bits are unknown bits. */
#define SBCE_LINEAR_EP_PASSES(n) (((n) & 0xff) << 8)

typedef struct sbce_linear_dims {
    int32_t batch;      /* B: independent trials (>= 1) */
    int32_t n_tx;       /* streams (1..8) */
    int32_t n_rx;       /* receive antennas (1..8; ZF: >= n_tx) */
    int32_t n_psi;      /* P = rows of PsiTilde_td (>= 1) */
    int32_t t_d;        /* data symbols (>= 1) */
    int32_t m;          /* table size (power of two, 2..64) */
    int32_t kind;       /* SBCE_LINEAR_* */
    int32_t flags;      /* SBCE_DETECT_MAXLOG, SBCE_LINEAR_EP_PASSES(n) (EP); every other bit 0 */
    double sigma2;      /* > 0: the denominator itself, as sbce_detect_dims.sigma2 */
    double es;          /* > 0: symbol energy of the MMSE / EP prior (mean |cons|^2; 1 gives the
                           reference's filter of all_detectorsvsTd.py:71); ignored by ZF */
} sbce_linear_dims;

typedef struct sbce_linear_ptrs {
    const void* y_d;
    const void* psi_d;
    const void* cons;
    const void* theta;
    const int32_t* labels;   /* may be NULL unless llr or err is set */
    const double* sigma2_t;  /* may be NULL: [B] per-trial sigma2 (values > 0) */
    const void* x_d_true;    /* may be NULL unless err is set */
    void* x_soft;            /* may be NULL */
    double* nu;              /* may be NULL */
    void* x_hat;             /* may be NULL */
    int32_t* idx_hat;        /* may be NULL */
    double* post;            /* may be NULL */
    double* llr;             /* may be NULL (requires labels) */
    int32_t* err;            /* may be NULL (requires x_d_true and labels); zeroed by the call */
    void* moments;           /* may be NULL */
    int32_t* status;         /* may be NULL: 0 or SBCE_STATUS_NONHPD; zeroed by the call */
    void* workspace;         /* may be NULL when the workspace query reports 0 */
    size_t workspace_bytes;
} sbce_linear_ptrs;

/* Device workspace of the linear detection call for `d` (0 in this version). */
int sbce_detect_linear_workspace_bytes(const sbce_linear_dims* d, size_t* bytes);

/* One pass over every (trial, data symbol): one small kernel that zeroes `err` and `status` (when
 * either is set; a kernel where the detector above uses a memset, so that a captured graph holds
 * kernel nodes only), then one kernel launch, in this order on `hip_stream`; no allocation, no
 * synchronisation, no floating-point atomic; capturable in a HIP graph.
 * Decided before any HIP call -- SBCE_EINVAL: null dims / ptrs / required pointer, batch, t_d,
 * n_psi, n_tx or n_rx < 1, m not a power of two in 2..64, sigma2 <= 0, MMSE or EP with es <= 0, an
 * unknown kind or flag bit, llr without labels, err without x_d_true or labels, ZF with
 * n_rx < n_tx, a misaligned pointer (16 bytes complex, 8 float64, 4 int32);
 * SBCE_EUNSUPPORTED: n_tx > 8 or n_rx > 8; SBCE_EWORKSPACE. */
int sbce_detect_linear(const sbce_linear_dims* d, const sbce_linear_ptrs* p, void* hip_stream);

/* ---- Cramer-Rao bounds and the predicted NMSE (an additive extension of ABI 7: no existing
 * struct or entry point changes).  In the reduced form y = H_c u + n, u = psi (x) x,
 * n ~ CN(0, sigma^2 I), the normal matrix of the M-step is
 *   R = sum_p u_p u_p^H + sum_t (psi_t psi_t^H) (x) S_t          (L x L, L = n_psi n_tx).
 * With the regressors known every row of the least-squares estimate has covariance sigma^2 R^-1,
 * so E||theta_hat - theta||^2 = n_rx sigma^2 tr(R^-1) -- also the Cramer-Rao bound -- and the
 * variance of coefficient (l, r) is sigma^2 (R^-1)_ll.  The moments given to the build select the
 * quantity: zero moments (S_t = 0) give the pilot-only bound; m_t = x_t, S_t = x_t x_t^H the bound
 * with all data known (the floor of every semi-blind curve); an E-step's moments the
 * complete-data error variance of the estimate made from them, which ignores the information lost
 * to symbol uncertainty and so is optimistic.
 * Per trial: R = G G^H, W = G^-1, diag_inv[l] = sum_{k >= l} |W_kl|^2, tr_inv = sum_l diag_inv[l].
 * Pivot rule (SBCE_SOLVE_CHOL's threshold): a Cholesky pivot that is not above 1e-14 max_l R_ll --
 * a NaN pivot included -- makes the trial unidentifiable: tr_inv, mse, bound and every diag_inv
 * entry of the trial are +inf and it gets SBCE_STATUS_NONHPD; other trials are unaffected.
 * Nothing is dropped or regularised: a bound on a subspace is not the bound. */
typedef struct sbce_crb_opts {
    double sigma2;           /* > 0: the noise variance the data carry (varn of the signal model,
                                NOT the posterior's varn^2) */
    const double* sigma2_t;  /* may be NULL: [B] per-trial values > 0, used instead of sigma2 */
    double* tr_inv;          /* [B] out: tr(R^-1) */
    double* diag_inv;        /* may be NULL: [B][L] out, (R^-1)_ll */
    double* mse;             /* may be NULL: [B] out, n_rx sigma_b^2 tr(R^-1) */
    double* bound;           /* may be NULL (requires p->h_true): [B] out, mse / ||h_true_b||^2 */
    void* scratch;           /* device scratch, 16-byte aligned */
    size_t scratch_bytes;    /* at least sbce_crb_workspace_bytes */
    int32_t flags;           /* 0 */
} sbce_crb_opts;

/* Device scratch of sbce_crb for `d` (the inverses of the factor's diagonal tiles, and the
 * discarded solution of the build launch at small L).  SBCE_EUNSUPPORTED as sbce_crb. */
int sbce_crb_workspace_bytes(const sbce_dims* d, size_t* bytes);

/* R is built from p->y_p, u_p, psi_d and `moments` (sbce_estep's layout; required) by the launches
 * of sbce_mstep's build into p->workspace (sized as for sbce_mstep with SBCE_SOLVE_CHOL), then one
 * kernel factors and inverts it in place: the call sees the R sbce_mstep reports in r_out, lower
 * triangle only.  p->theta, y_d, y_p and `moments` are never written; p->status, when set, is
 * written (0, SBCE_STATUS_PILOT from the build, SBCE_STATUS_NONHPD).  d, p and `moments` are checked
 * as sbce_mstep checks them.  No allocation, no synchronisation, no floating-point atomic; every
 * order of summation is fixed by (L, n_rx) alone, so trial b of a B-trial call is bitwise the
 * B = 1 call, whatever the workspace held; capturable in a HIP graph as a linear chain.
 * Decided before any HIP call, beside sbce_mstep's own -- SBCE_EINVAL: null o, tr_inv or scratch,
 * a misaligned pointer (8 bytes float64, 16 bytes scratch), sigma2 <= 0, bound without p->h_true,
 * flags != 0; SBCE_EUNSUPPORTED: L = n_psi n_tx > 512 (the tiled large-L factorisation has no
 * inverse yet); SBCE_EWORKSPACE: scratch_bytes too small. */
int sbce_crb(const sbce_dims* d, const sbce_ptrs* p, const void* moments,
             const sbce_crb_opts* o, void* hip_stream);

/* ---- Soft-input EP detection and code-aided EM: a-priori bit L-values (an additive extension of
 * ABI 7: no existing struct or entry point changes).  Every E-step and detector above assumes
 * equiprobable data symbols; the three calls below take what a decoder hands back to the front
 * end, la [B][T_d][n_tx][log2 M] float64 with La = log(P(bit = 0) / P(bit = 1)) -- the sign
 * convention of the llr outputs -- and bit_i(s) = (labels[s] >> i) & 1.  On load each value is
 * sanitised: NaN becomes 0 and anything outside +-64 (kPriorClamp) is clamped to +-64, so +-inf
 * means a known bit.
 * Per (b, t), with H, G, u, s2 and es as for SBCE_ESTEP_EP / SBCE_LINEAR_EP:
 *   prior   lp_a[s] = -sum_i bit_i(s) La[a][i], shifted so that its largest member is 0;
 *           pi_a = softmax(lp_a) (formed max-shifted: one weight is 1); prior mean
 *           xbar_a = sum pi cons, prior variance v0_a = max(sum pi |cons|^2 - |xbar_a|^2,
 *           kEpVarFloor es)
 *   start   r_a = s2 / v0_a,  q_a = s2 xbar_a / v0_a
 *   pass l = 1..p   the solve, the pivot rule and the cavity (t_a, h2_a) are those of
 *           SBCE_ESTEP_EP; the demapper weights are e^{-|t_a - cons[s]|^2 / h2_a + lp_a[s]},
 *           shifted by the largest exponent so that one weight is 1; the state update is
 *           unchanged: v = max(s_a - |m_a|^2, floor), r' = s2 (1/v - 1/h2), q' = s2 (m/v - t/h2),
 *           damping 0.5, kept when r' is not finite and positive
 *   outputs of the last pass   x_soft = t and nu = h2: the extrinsic estimate (stream a's own
 *           prior is not in them); post = the a-posteriori pmf, prior included; moments in the
 *           product form, from post (what the E-step stores); idx_hat = argmax_s (-d_s / h2 +
 *           lp[s]), ties to the lowest s, x_hat = cons[idx_hat]; llr[a][i] = L_post - La (the
 *           sanitised value), the EXTRINSIC L-value, L_post the class log-sum difference over the
 *           prior-weighted exponents (SBCE_DETECT_MAXLOG: the max-log form of the same exponents,
 *           minus La); err is counted as in sbce_detect_linear.
 * One pass (p = 1) is the classical soft-interference-cancellation MMSE turbo detector.
 * Degenerate cases: a failed pivot in any pass makes every stream of the symbol channel-blind:
 * x_soft = 0, nu = +inf, post = pi_a, moments from pi_a, llr = 0, and the status bit of the
 * prior-free call; a stream with mu_a <= 0 gets the same for itself alone.  Every output stays
 * finite for any s2 > 0 and any bit pattern of la.
 * Determinism: summation orders are fixed by (n_tx, n_rx, n_psi, m, p); trial b of a B-trial call
 * is bitwise the B = 1 call; there are no floating-point atomics.
 * No prior (la == NULL, or pr == NULL): each call IS the existing call -- sbce_detect_linear,
 * sbce_estep, sbce_em / sbce_em_noise / sbce_em_conv -- with the same launches and the same bits.
 * With a prior only SBCE_LINEAR_EP and SBCE_ESTEP_EP are accepted (pass counts carried as there);
 * any other kind or mode, and cv->ll_hist together with a prior, is SBCE_EUNSUPPORTED.
 * SBCE_EINVAL, decided before any HIP call: la without labels, a misaligned la (8 bytes) or labels
 * (4 bytes), flags != 0, p->x_sup set, and every check of the wrapped call.
 * No allocation, no synchronisation; capturable in a HIP graph as a linear chain of kernel nodes;
 * the launch counts are those of the prior-free call. */
typedef struct sbce_prior_opts {
    const double*  la;      /* [B][T_d][n_tx][log2 M]; NULL: no prior */
    const int32_t* labels;  /* [M], a permutation of 0..M-1; required when la is set */
    int32_t flags;          /* 0 */
} sbce_prior_opts;

/* sbce_detect_linear with the prior la; the labelling is p->labels. */
int sbce_detect_linear_prior(const sbce_linear_dims* d, const sbce_linear_ptrs* p,
                             const double* la, void* hip_stream);
/* sbce_estep with the prior pr. */
int sbce_estep_prior(const sbce_dims* d, const sbce_ptrs* p, int estep_mode,
                     const sbce_prior_opts* pr, void* moments, void* hip_stream);
/* sbce_em (nz == NULL, cv == NULL), sbce_em_noise (nz) or sbce_em_conv (cv, nz may be NULL) with
 * the prior pr, constant over the iterations. */
int sbce_em_prior(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
                  const sbce_prior_opts* pr, const sbce_noise_opts* nz, const sbce_conv_opts* cv,
                  void* hip_stream);

/* ---- Soft-in / soft-out channel decoder (an additive extension of ABI 7: no existing struct or
 * entry point changes): exact log-MAP (BCJR) decoding of a batch of codewords of one binary code,
 * the block that produces the a-priori L-values the section above consumes.  Every L-value here is
 * L = log(P(bit = 0) / P(bit = 1)), the convention of llr and la above.
 * Code: rate 1/n, feed-forward, non-systematic; n in {2, 3}; constraint length K in 3..7, so
 * S = 2^(K-1) states.  The generators g_j are K-bit integers whose bit K-1 taps the current input;
 * bit K-1 and bit 0 of every generator must be set and no bit above K-1 (gen[2] is ignored at
 * n = 2).  State s = (u_{t-1}, ..., u_{t-K+1}) with u_{t-1} at bit K-2; register word
 * w = (u_t << (K-1)) | s; output c_j = parity(w & g_j); next state s' = w >> 1; the start state is
 * 0.  With SBCE_SISO_TERMINATED n_steps = n_info + K - 1, the K - 1 tail inputs are forced to 0
 * and the end state is 0; without it n_steps = n_info and every end state is allowed.
 * Known answer: g = (7, 5) octal, u = 1011, terminated: the codeword is 11 10 00 01 01 11.
 * Inputs: lc [B][n_steps n] float64, coded bit k = t n + j; la_u [B][n_info] (may be NULL: 0);
 * perm int32 [n_steps n] (may be NULL: the identity), a bijection of 0 .. n_steps n - 1 -- the
 * caller's contract, not checked: coded bit k is read from lc[b][perm[k]] and its extrinsic value
 * written to le_c[b][perm[k]], so the de-interleaver and the interleaver cost no launch.  Every
 * L-value is sanitised on load as la above: NaN becomes 0, values outside +-64 are clamped.
 * Recursion, with Lc and La the sanitised values:
 *   gamma_t(s, u) = -sum_j c_j(s, u) Lc[t][j] - u La[t]; the branch u = 1 does not exist at tail
 *   steps.  alpha_0(0) = 0, else -inf; alpha_{t+1}(s') = lse over the two branches into s';
 *   beta_{n_steps} = 0 at every allowed end state, else -inf; beta_t(s) = lse over the branches
 *   out of s; A_t(s, u) = alpha_t(s) + gamma_t(s, u) + beta_{t+1}(s').
 * Outputs (each may be NULL, at least one is required):
 *   lapp_u[b][t]   lse_{u = 0} A_t - lse_{u = 1} A_t, t < n_info: the a-posteriori L-value
 *   u_hat[b][t]    int32 [lapp_u < 0]; a tie gives 0
 *   le_c[b][k]     (lse_{c_j = 0} A_t - lse_{c_j = 1} A_t) - Lc[t][j]: the EXTRINSIC L-value of
 *                  coded bit k = t n + j, tail steps included, at position perm[k]
 *   err[b]         int32: bit errors of u_hat against u_true (integer adds; zeroed by the call)
 * With SBCE_DETECT_MAXLOG every lse above is a max (max-log-MAP).
 * Numerical rules: every lse is shifted by the maximum of its own members; -inf is an ordinary
 * value and lse of nothing but -inf is -inf.  An output is +-inf exactly when one of its two
 * classes is empty, which (the sanitised inputs being finite) is a property of (code, t,
 * termination) alone: lapp_u is always finite (both inputs leave every reachable state and reach
 * an allowed end), le_c is infinite where every surviving path agrees on the coded bit -- g =
 * (7, 5), n_info = 1, terminated: step 1 is entered in states 0 and 2 only and g = 5 gives 0 on
 * both branches, so le_c[3] = +inf.  No output is NaN for any bit pattern of the inputs.  The metric rows are normalised by a fixed rule (each
 * stored row minus state 0's metric of the row it was formed from), which cancels in every output.
 * Determinism: no floating-point atomic; every order of summation is fixed by (K, n, n_steps,
 * flags); codeword b of a B-codeword call is bitwise the B = 1 call, whatever the workspace held. */
#define SBCE_SISO_TERMINATED 2  /* sbce_siso_dims.flags bit 1 (bit 0 is SBCE_DETECT_MAXLOG) */

typedef struct sbce_siso_dims {
    int32_t batch;      /* B: codewords (>= 1) */
    int32_t n_info;     /* information bits per codeword (>= 1) */
    int32_t k;          /* constraint length K (3..7) */
    int32_t n;          /* coded bits per step (2..3) */
    int32_t gen[3];     /* generators g_0 .. g_{n-1} */
    int32_t flags;      /* SBCE_DETECT_MAXLOG, SBCE_SISO_TERMINATED; every other bit 0 */
} sbce_siso_dims;

typedef struct sbce_siso_ptrs {
    const double*  lc;       /* [B][n_steps n] */
    const double*  la_u;     /* may be NULL: [B][n_info] */
    const int32_t* perm;     /* may be NULL: [n_steps n] */
    const int32_t* u_true;   /* may be NULL unless err is set: [B][n_info], 0 / 1 */
    double*  lapp_u;         /* may be NULL: [B][n_info] */
    int32_t* u_hat;          /* may be NULL: [B][n_info] */
    double*  le_c;           /* may be NULL: [B][n_steps n] */
    int32_t* err;            /* may be NULL (requires u_true): [B]; zeroed by the call */
    void* workspace;         /* the alpha and beta rows of the call, 16-byte aligned */
    size_t workspace_bytes;
} sbce_siso_ptrs;

/* Device workspace of the decoder for `d`: 512 n_steps bytes per group of 64 / S codewords.
 * Errors as sbce_siso_decode's checks of d. */
int sbce_siso_workspace_bytes(const sbce_siso_dims* d, size_t* bytes);

/* One decode is one kernel launch on `hip_stream`, preceded by one small kernel that zeroes `err`
 * when it is set; no allocation, no synchronisation; capturable in a HIP graph as a linear chain
 * of kernel nodes.
 * Decided before any HIP call, in this order -- SBCE_EINVAL: null d / p / lc, batch or n_info < 1,
 * an unknown flag bit; SBCE_EUNSUPPORTED: k outside 3..7 or n outside 2..3; SBCE_EINVAL: a
 * generator without bit K-1 or bit 0, or with a bit above K-1; SBCE_EUNSUPPORTED:
 * n_steps > 16384; SBCE_EINVAL: err without u_true, no output requested, a null workspace, a
 * misaligned pointer (8 bytes float64, 4 int32, 16 workspace); SBCE_EWORKSPACE: workspace_bytes
 * too small. */
int sbce_siso_decode(const sbce_siso_dims* d, const sbce_siso_ptrs* p, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SBCE_H_ */
