// extern "C" entry points of libsbce.so (declared in include/sbce.h).
//
// The EM loop replaces em() of "Proposed method/Proposed_method_NMSEvsTp.py":50-83
// for a whole batch of Monte-Carlo trials: per iteration one E-step launch over
// every (trial, symbol), one normal-equation build and one batched Cholesky
// solve, all stream-ordered, with no host synchronisation and no allocation.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "sbce_internal.h"

using namespace sbce;

namespace sbce {

#if SBCE_AB
DebugConfig g_debug;

namespace {
void read_debug_env(DebugConfig& c) {
    c = kDebugDefault;
    auto env = [](const char* n) { const char* v = getenv(n); return (v && v[0]) ? v : nullptr; };
    const char* v;
    if ((v = env("SBCE_ESTEP_IMPL"))) c.estep_valu = v[0] == 'v';
    if ((v = env("SBCE_ESTEP_PRUNE"))) c.estep_noprune = v[0] == '0';
    if ((v = env("SBCE_ESTEP_COUNT"))) c.estep_count = v[0] == '1';
    if ((v = env("SBCE_ESTEP_F32"))) c.estep_nof32 = v[0] == '0';
    if ((v = env("SBCE_ESTEP_SPHERE"))) c.estep_nosphere = v[0] == '0';
    if ((v = env("SBCE_SPHERE_BUDGET"))) {
        const int bu = atoi(v);
        c.sphere_budget = bu < 1 ? 1 : (bu > kBfsPmax ? kBfsPmax : bu);
    }
    if ((v = env("SBCE_BACKSUB"))) c.backsub_general = v[0] == '1';
    if ((v = env("SBCE_CHOL_IMPL"))) c.chol_valu = v[0] == 'v';
    if ((v = env("SBCE_ESTEP_PAIR"))) c.estep_nopair = v[0] == '0';
    if ((v = env("SBCE_CPLX3"))) c.cplx3 = v[0] != '0';
    if ((v = env("SBCE_MSTEP_SMALL"))) {
        c.mstep_nosmall = v[0] == '0';
        c.small_valu = v[0] == 'v';
        c.small_v1 = v[0] == '1';
    }
    if ((v = env("SBCE_PM_IMPL"))) c.pm_impl = (v[0] == 'w' || v[0] == 't' || v[0] == 'q') ? v[0] : 0;
    if ((v = env("SBCE_SMALL_SOLVE"))) c.small_col = v[0] == 'c';
    if ((v = env("SBCE_ESTEP_TRI"))) c.estep_tri = (v[0] >= '0' && v[0] <= '2') ? v[0] - '0' : 1;
    if ((v = env("SBCE_ESTEP_ORDER"))) c.estep_noorder = v[0] == '0';
    if ((v = env("SBCE_ESTEP_TWOPASS"))) c.estep_notwopass = v[0] == '0';
    if ((v = env("SBCE_SMALL_STOP"))) c.small_stop = (v[0] >= '1' && v[0] <= '4') ? v[0] - '0' : 0;
}

__attribute__((constructor)) void load_debug_env() { read_debug_env(g_debug); }
}  // namespace

bool debug_nondefault() {
    const DebugConfig& c = g_debug;
    const DebugConfig& d = kDebugDefault;
    return c.estep_valu != d.estep_valu || c.estep_noprune != d.estep_noprune ||
           c.estep_nof32 != d.estep_nof32 || c.estep_tri != d.estep_tri || c.estep_noorder != d.estep_noorder ||
           c.estep_notwopass != d.estep_notwopass ||
           c.estep_nosphere != d.estep_nosphere || c.sphere_budget != d.sphere_budget ||
           c.backsub_general != d.backsub_general || c.chol_valu != d.chol_valu ||
           c.estep_nopair != d.estep_nopair || c.cplx3 != d.cplx3 ||
           c.mstep_nosmall != d.mstep_nosmall || c.small_stop != d.small_stop ||
           c.small_valu != d.small_valu || c.small_v1 != d.small_v1 || c.small_col != d.small_col ||
           (chol_debug_skip_mask() & 31);
}
#else
bool debug_nondefault() { return false; }   // the product build has no switch
#endif

}  // namespace sbce

namespace {

constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Carve {
    size_t mom, R, rhs, done, mchg, ysh, prep, list, tree, tol, winv, ppsi, pS, pflag, prhs, gram, grhs,
        act, tol2, dvec, mnr, mnskip, total;
    bool has_prep, has_prhs, has_winv, has_mn;
};

constexpr int kAnySolve = -1;            // carve for every solve mode (sbce_workspace_bytes)

bool make_problem(const sbce_dims* d, Problem& pb) {
    if (!d) return false;
    if (d->batch < 0 || d->n_tx < 1 || d->n_rx < 1 || d->n_psi < 1 || d->t_p < 0 || d->t_d < 1 ||
        d->m < 2 || d->partition_r < 0 || !(d->varn > 0.0))
        return false;
    if (d->n_tx > 8 || d->n_rx > 8) return false;
    pb.B = d->batch; pb.NT = d->n_tx; pb.NR = d->n_rx; pb.P = d->n_psi;
    pb.Tp = d->t_p; pb.Td = d->t_d; pb.M = d->m; pb.varn = d->varn; pb.pr = d->partition_r;
    pb.varx = d->varx;
    pb.L = pb.P * pb.NT;
    pb.K = pb.L * pb.NR;
    return true;
}

// Workspace layout for `solve` (SBCE_SOLVE_*, or kAnySolve): the regions only the tiled
// factorisation (L > 512) or the min-norm solve use are appended last and carved only when that
// solve can run, so a CHOL workspace at L <= 512 holds no Gram matrix.  Offsets of every region
// that is carved do not depend on `solve`.
Carve carve(const Problem& pb, int solve = kAnySolve) {
    Carve c;
    const size_t MS = (size_t)pb.NT + (size_t)pb.NT * pb.NT;
    c.mom = 0;
    c.R = align_up(c.mom + (size_t)pb.B * pb.Td * MS * sizeof(cd));
    c.rhs = align_up(c.R + (size_t)pb.B * pb.L * pb.L * sizeof(cd));
    c.done = align_up(c.rhs + (size_t)pb.B * pb.L * pb.NR * sizeof(cd));
    c.ysh = align_up(c.done + (size_t)pb.B * sizeof(int32_t));         // superimposed pilots
    // the moment-repeat words [B] int32 (em_run) share the head of the shifted observations: the
    // rule is never armed with superimposed pilots, and the region holds >= 16 bytes per trial
    c.mchg = c.ysh;
    c.prep = align_up(c.ysh + (size_t)pb.B * pb.Td * pb.NR * sizeof(cd));   // MFMA sweep prep
    const int ps = estep_prep_stride(pb);
    c.has_prep = ps > 0;
    c.list = align_up(c.prep + (size_t)pb.B * pb.Td * ps * sizeof(double));
    c.tree = align_up(c.list + (3 * (size_t)pb.B * pb.Td + 2 * kEstepListCnt) * sizeof(int32_t));
    c.tol = c.has_prep ? align_up(c.tree + (size_t)pb.B * pb.Td * kTreeRecDoubles * sizeof(double))
                       : c.list;
    c.ppsi = c.pS = c.pflag = c.winv = c.tol;
    c.total = c.tol;
    if (rbuild_herm_supported(pb)) {         // MFMA R build: Kronecker-factored pilots
        c.ppsi = c.total;
        c.pS = align_up(c.ppsi + (size_t)pb.B * pb.Tp * pb.P * sizeof(cd));
        c.pflag = align_up(c.pS + (size_t)pb.B * pb.Tp * pb.NT * pb.NT * sizeof(cd));
        c.total = align_up(c.pflag + (size_t)pb.B * sizeof(int32_t));
    }
    // the pilot part of B^H is fixed across iterations: kept once per run for the L <= 512
    // B^H kernel (mstep.hip rhs_dma_kernel), which then reads L*NR values instead of u_p, y_p
    c.has_prhs = rbuild_herm_supported(pb) && pb.L <= kLargeL;
    c.prhs = c.total;
    if (c.has_prhs) c.total = align_up(c.prhs + (size_t)pb.B * pb.L * pb.NR * sizeof(cd));
    c.tol = c.total;                         // per-trial pivot threshold
    c.winv = align_up(c.tol + (size_t)pb.B * sizeof(double));
    c.total = c.winv;
    c.has_mn = solve == kAnySolve || solve == SBCE_SOLVE_MINNORM;
    // tiled factorisation (L > 512, and the min-norm solve at every L): diagonal-tile inverse
    c.has_winv = c.has_mn || pb.L > kLargeL;
    c.gram = c.winv;
    if (c.has_winv) c.total = c.gram = align_up(c.winv + (size_t)pb.B * 64 * 64 * sizeof(cd));
    c.grhs = c.act = c.tol2 = c.dvec = c.mnr = c.mnskip = c.total;
    if (c.has_mn) {
        // min-norm solve (minnorm.hip): Gram matrix C = G^H G, its right-hand sides, extents
        c.grhs = align_up(c.gram + (size_t)pb.B * pb.L * pb.L * sizeof(cd));
        c.act = align_up(c.grhs + (size_t)pb.B * pb.L * pb.NR * sizeof(cd));
        c.tol2 = align_up(c.act + (size_t)pb.B * sizeof(int32_t));
        c.dvec = align_up(c.tol2 + (size_t)pb.B * sizeof(double));
        // one refinement step on the kept subspace: residual and per-trial gate
        c.mnr = align_up(c.dvec + (size_t)pb.B * pb.L * sizeof(double));
        c.mnskip = align_up(c.mnr + (size_t)pb.B * pb.L * pb.NR * sizeof(cd));
        c.total = align_up(c.mnskip + (size_t)pb.B * sizeof(int32_t));
    }
    return c;
}

int hip_rc(hipError_t e) { return e == hipSuccess ? SBCE_OK : SBCE_EHIP; }

// The launchers check their kernels with hipGetLastError(), which reports the last error of ANY
// HIP call on this host thread until it is read.  A caller's earlier failed or "not ready" call
// (e.g. an event query by the framework that owns the buffers) must not be reported as a failure
// of this library's launches: every entry point that launches clears it first.
void clear_stale_error() { (void)hipGetLastError(); }

void set_large(MstepArgs& ma, char* ws, const Carve& c) {
    ma.tol = (double*)(ws + c.tol);
    ma.winv = c.has_winv ? (cd*)(ws + c.winv) : nullptr;
    ma.ppsi = (cd*)(ws + c.ppsi);
    ma.pS = (cd*)(ws + c.pS);
    ma.pflag = (int32_t*)(ws + c.pflag);
    ma.prhs = c.has_prhs ? (cd*)(ws + c.prhs) : nullptr;
    ma.gate = nullptr;
    ma.gram = c.has_mn ? (cd*)(ws + c.gram) : nullptr;
    ma.grhs = c.has_mn ? (cd*)(ws + c.grhs) : nullptr;
    ma.act = c.has_mn ? (int32_t*)(ws + c.act) : nullptr;
    ma.tol2 = c.has_mn ? (double*)(ws + c.tol2) : nullptr;
    ma.dvec = c.has_mn ? (double*)(ws + c.dvec) : nullptr;
    ma.mnr = c.has_mn ? (cd*)(ws + c.mnr) : nullptr;
    ma.mnskip = c.has_mn ? (int32_t*)(ws + c.mnskip) : nullptr;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// every pointer of the list is non-null and 16-byte aligned
bool required(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if (!q || !aligned16(q)) return false;
    return true;
}

bool valid_solve(int mode) {
    return mode == SBCE_SOLVE_CHOL || mode == SBCE_SOLVE_CHOL_DROP || mode == SBCE_SOLVE_MINNORM;
}

// The M-step's arguments from the caller's buffers, the given moments and the workspace carved
// by `c` (for `solve`); no status gate (done) -- em_run sets its own.
MstepArgs mstep_args(const Problem& pb, const sbce_ptrs* p, const void* moments, char* ws,
                     const Carve& c, int solve) {
    MstepArgs ma;
    ma.yd = (const cd*)p->y_d; ma.yp = (const cd*)p->y_p; ma.psid = (const cd*)p->psi_d;
    ma.up = (const cd*)p->u_p; ma.mom = (const cd*)moments; ma.R = (cd*)(ws + c.R);
    ma.rhs = (cd*)(ws + c.rhs); ma.theta = (cd*)p->theta; ma.status = p->status; ma.done = nullptr;
    ma.solve_mode = solve; ma.nbatch = pb.B;
    set_large(ma, ws, c);
    return ma;
}

// SBCE_ESTEP_MMSE_SOFT / ZF_SOFT / EP report n_tx or n_rx past 8 as SBCE_EUNSUPPORTED, like
// sbce_detect_linear, whose arithmetic they are (include/sbce.h); make_problem alone would say
// SBCE_EINVAL, which stays the answer for every other mode.
bool linear_oversize(const sbce_dims* d, int estep_mode) {
    return d && (estep_linear_mode(estep_mode) || estep_mode == SBCE_ESTEP_EP) && d->n_tx >= 1 && d->n_rx >= 1 &&
           (d->n_tx > 8 || d->n_rx > 8);
}

// SBCE_ESTEP_EP reads partition_r as its pass count: 0 (the default) .. 16
bool ep_passes_invalid(const Problem& pb, int estep_mode) {
    return estep_mode == SBCE_ESTEP_EP && ep_passes_of(pb.pr) < 0;
}

// The E-step's arguments: moments out, and the MFMA sweep's regions of the workspace carved by
// `c` (null: no workspace, the sweep kernel prepares each symbol itself).
EstepArgs estep_args(const sbce_ptrs* p, void* moments, char* ws, const Carve* c) {
    EstepArgs ea;
    ea.yd = (const cd*)p->y_d; ea.psid = (const cd*)p->psi_d; ea.theta = (const cd*)p->theta;
    ea.cons = (const cd*)p->cons; ea.mom = (cd*)moments; ea.done = nullptr;
    ea.status = p->status;
    ea.varn_t = p->varn_t;
    const bool prep = c && c->has_prep;
    ea.prep = prep ? (double*)(ws + c->prep) : nullptr;
    ea.list = prep ? (int32_t*)(ws + c->list) : nullptr;
    ea.tree = prep ? (double*)(ws + c->tree) : nullptr;
    return ea;
}

// per-trial status starts at 0, or at SBCE_STATUS_DEBUG while a result-affecting debug switch
// (DebugConfig) is active
int status_init(int32_t* status, int B, hipStream_t s) {
    if (!status) return SBCE_OK;
    const unsigned v = debug_nondefault() ? SBCE_STATUS_DEBUG : 0u;
    return hipMemsetD32Async((hipDeviceptr_t)status, v, (size_t)B, s) == hipSuccess ? SBCE_OK
                                                                                    : SBCE_EHIP;
}

int check_ptrs(const sbce_ptrs* p, const Problem& pb, bool need_ws, int solve = kAnySolve) {
    if (!p) return SBCE_EINVAL;
    if (!required({p->y_d, p->y_p, p->psi_d, p->u_p, p->cons, p->theta})) return SBCE_EINVAL;
    if (p->varn_t && ((uintptr_t)p->varn_t & 7)) return SBCE_EINVAL;
    if (need_ws) {
        if (!p->workspace || !aligned16(p->workspace)) return SBCE_EINVAL;
        if (p->workspace_bytes < carve(pb, solve).total) return SBCE_EWORKSPACE;
    }
    return SBCE_OK;
}

// sbce_noise_opts against `pb` (sbce_noise_var, sbce_em_noise): decided before any HIP call
size_t noise_scratch_bytes(const Problem& pb) {
    return align_up((size_t)pb.B * noise_nblk(pb) * sizeof(double));
}

int check_noise(const sbce_ptrs* p, const sbce_noise_opts* o, const Problem& pb) {
    if (!p || !o) return SBCE_EINVAL;
    if (p->x_sup || p->llf) return SBCE_EINVAL;
    if (!o->varn_est || ((uintptr_t)o->varn_est & 7) || ((uintptr_t)o->varn_hist & 7))
        return SBCE_EINVAL;
    if (!(o->varn_min > 0.0) || o->flags != 0) return SBCE_EINVAL;
    if (!o->scratch || ((uintptr_t)o->scratch & 7)) return SBCE_EINVAL;
    if (o->scratch_bytes < noise_scratch_bytes(pb)) return SBCE_EWORKSPACE;
    return SBCE_OK;
}

// One noise update: the block sums of Q, then the per-trial rules.  fin (stand-alone call): the
// previous value and the status word's base; null (inside the EM loop): the previous value is
// varn_est itself, the flag is OR-ed into the status word and varn_hist[b][it] is written.
int noise_update(const Problem& pb, const sbce_ptrs* p, const cd* mom, const int32_t* done,
                 const sbce_noise_opts* o, const NoiseFinalArgs* fin, int iters, int it,
                 hipStream_t s) {
    NoiseArgs a{};
    a.yd = (const cd*)p->y_d; a.yp = (const cd*)p->y_p; a.psid = (const cd*)p->psi_d;
    a.up = (const cd*)p->u_p; a.theta = (const cd*)p->theta; a.mom = mom; a.done = done;
    a.part = (double*)o->scratch;
    int rc = hip_rc(launch_noise_partial(pb, a, s));
    if (rc) return rc;
    NoiseFinalArgs f{};
    if (fin) {
        f = *fin;
    } else {
        f.prev_t = o->varn_est;
        f.status_base = -1;
        f.hist = o->varn_hist;
    }
    f.part = a.part; f.done = done; f.varn_est = o->varn_est; f.status = p->status;
    f.varn_min = o->varn_min; f.iters = iters; f.it = it;
    return hip_rc(launch_noise_final(pb, f, s));
}

// sbce_crb's scratch: the diagonal tiles' inverses, then the theta the small-L build launch solves
// for (discarded)
size_t crb_scratch_bytes(const Problem& pb) {
    return align_up(crb_dinv_bytes(pb)) + align_up((size_t)pb.B * pb.K * sizeof(cd));
}

// the log-likelihood's scratch: per-symbol terms (used when the caller takes no ll_sym), then the
// pilot block sums
size_t loglik_sym_bytes(const Problem& pb) {
    return align_up((size_t)pb.B * pb.Td * sizeof(double));
}
size_t loglik_scratch_bytes(const Problem& pb) {
    return loglik_sym_bytes(pb) + align_up((size_t)pb.B * loglik_npb(pb) * sizeof(double));
}

LoglikArgs loglik_args(const Problem& pb, const sbce_ptrs* p, double* ll, double* ll_sym,
                       char* scratch) {
    LoglikArgs a{};
    a.yd = (const cd*)p->y_d; a.yp = (const cd*)p->y_p; a.psid = (const cd*)p->psi_d;
    a.up = (const cd*)p->u_p; a.cons = (const cd*)p->cons; a.theta = (const cd*)p->theta;
    a.varn_t = p->varn_t;
    a.sym = ll_sym ? ll_sym : (double*)scratch;
    a.ppart = (double*)(scratch + loglik_sym_bytes(pb));
    a.ll = ll;
    return a;
}

// the convergence stop's scratch: theta_prev, the iteration's ll, then the log-likelihood's own
size_t conv_prev_bytes(const Problem& pb) { return align_up((size_t)pb.B * pb.K * sizeof(cd)); }
size_t conv_ll_bytes(const Problem& pb) { return align_up((size_t)pb.B * sizeof(double)); }
size_t conv_scratch_bytes(const Problem& pb, bool want_ll) {
    return conv_prev_bytes(pb) + conv_ll_bytes(pb) + (want_ll ? loglik_scratch_bytes(pb) : 0);
}

// sbce_conv_opts against `pb` (sbce_em_conv): decided before any HIP call
int check_conv(const sbce_ptrs* p, const sbce_conv_opts* cv, const Problem& pb) {
    if (!p || !cv) return SBCE_EINVAL;
    if (p->h_true || p->llf || p->x_sup) return SBCE_EINVAL;
    if (!(cv->tol_theta >= 0.0) || !(cv->tol_ll >= 0.0) || cv->min_iters < 1 || cv->flags != 0)
        return SBCE_EINVAL;
    if (cv->tol_ll > 0.0 && !cv->ll_hist) return SBCE_EINVAL;
    if (((uintptr_t)cv->dtheta_hist & 7) || ((uintptr_t)cv->ll_hist & 7)) return SBCE_EINVAL;
    if (!cv->scratch || !aligned16(cv->scratch)) return SBCE_EINVAL;
    if (cv->ll_hist && !loglik_supported(pb)) return SBCE_EUNSUPPORTED;
    if (cv->scratch_bytes < conv_scratch_bytes(pb, cv->ll_hist != nullptr)) return SBCE_EWORKSPACE;
    return SBCE_OK;
}

// sbce_prior_opts (sbce_estep_prior, sbce_em_prior) after the wrapped call's own checks; *on = a
// prior is given.  pr == NULL or la == NULL: the call is the wrapped call.
int check_prior(const sbce_ptrs* p, const sbce_prior_opts* pr, int estep_mode, bool* on) {
    *on = false;
    if (!pr) return SBCE_OK;
    if (pr->flags != 0) return SBCE_EINVAL;
    if (!pr->la) return SBCE_OK;
    if (!pr->labels || ((uintptr_t)pr->la & 7) || ((uintptr_t)pr->labels & 3)) return SBCE_EINVAL;
    if (p->x_sup) return SBCE_EINVAL;
    if (estep_mode != SBCE_ESTEP_EP) return SBCE_EUNSUPPORTED;
    *on = true;
    return SBCE_OK;
}

}  // namespace

extern "C" {

int sbce_abi_version(void) { return SBCE_ABI_VERSION; }

const char* sbce_strerror(int code) {
    switch (code) {
        case SBCE_OK: return "ok";
        case SBCE_EINVAL: return "invalid argument (dims, null or misaligned pointer)";
        case SBCE_EUNSUPPORTED: return "shape not supported by the compiled kernel set";
        case SBCE_EHIP: return "HIP launch failed";
        case SBCE_EWORKSPACE: return "workspace too small";
    }
    return "unknown error";
}

int sbce_workspace_bytes(const sbce_dims* d, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb)) return SBCE_EINVAL;
    *bytes = carve(pb).total;
    return SBCE_OK;
}

int sbce_workspace_bytes_solve(const sbce_dims* d, int solve_mode, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb) || !valid_solve(solve_mode)) return SBCE_EINVAL;
    *bytes = carve(pb, solve_mode).total;
    return SBCE_OK;
}

}  // extern "C"

namespace {

// The EM loop of sbce_em, sbce_em_noise, sbce_em_conv and sbce_em_multi as a chain on one struct:
// check() decides everything that needs no HIP call, begin() issues what precedes the loop,
// iteration(it) one iteration, finish() the decisions launch and the iters_done fill.
// nz == nullptr: sbce_em.  nz: the noise parameter is estimated (noise.hip): nz->varn_est is the
// E-step's per-trial parameter, updated after every M-step, and the oracle early stop runs after
// the update in its own launch.  cv: the truth-free stop (loglik.hip) closes every iteration and
// owns the `done` flags; with cv absent the launches are exactly those of the loop without it.
struct EmChain {
    const sbce_ptrs* p = nullptr;
    const sbce_noise_opts* nz = nullptr;
    const sbce_conv_opts* cv = nullptr;
    const sbce_prior_opts* pr = nullptr;     // a-priori L-values of the data symbols, or null
    int iters = 0, estep_mode = 0, solve_mode = 0;
    hipStream_t s = nullptr;
    Problem pb;
    Carve c;
    char* ws = nullptr;
    int32_t* done = nullptr;
    int32_t* list_cnt = nullptr;
    int32_t* mchg = nullptr;
    bool empty = true;                       // no trial or no iteration: nothing is issued
    bool gauss = false, early = false, small = false, small2 = false, freeze = false,
         momfreeze = false, prefactor = false, fold_stop = false;
    EstepArgs ea, eas;
    MstepArgs ma;
    ConvArgs ca{};
    LoglikArgs la{};
    // the all-frozen report (MstepArgs::report and what em_init_kernel writes to its block), set
    // before begin() by a paced sbce_em_multi problem; only with `freeze`
    FreezeReport* rep = nullptr;
    int32_t* rep_word = nullptr;
    int32_t rep_gen = 0;

    int check(const sbce_dims* d, const sbce_ptrs* p_, int iters_, int estep_mode_, int solve_mode_,
              const sbce_noise_opts* nz_, const sbce_conv_opts* cv_, void* hip_stream,
              const sbce_prior_opts* pr_ = nullptr) {
        p = p_; nz = nz_; cv = cv_;
        iters = iters_; estep_mode = estep_mode_; solve_mode = solve_mode_;
        s = (hipStream_t)hip_stream;
        if (linear_oversize(d, estep_mode)) return SBCE_EUNSUPPORTED;
        if (!make_problem(d, pb) || iters < 0) return SBCE_EINVAL;
        if (ep_passes_invalid(pb, estep_mode)) return SBCE_EINVAL;
        if ((nz || cv) && estep_mode == SBCE_ESTEP_GAUSS) return SBCE_EUNSUPPORTED;
        if (!estep_supported(pb, estep_mode) || !chol_supported(pb)) return SBCE_EUNSUPPORTED;
        if (!valid_solve(solve_mode)) return SBCE_EINVAL;
        int rc = check_ptrs(p, pb, true, solve_mode);
        if (rc) return rc;
        if (p->llf && !p->x_d_true) return SBCE_EINVAL;
        gauss = estep_mode == SBCE_ESTEP_GAUSS;
        if (gauss && !(pb.varx > 0.0)) return SBCE_EINVAL;
        const bool hard = estep_mode == SBCE_ESTEP_HARD || estep_mode == SBCE_ESTEP_ZF ||
                          estep_mode == SBCE_ESTEP_MMSE;
        if (p->x_dest && (!hard || !aligned16(p->x_dest))) return SBCE_EINVAL;
        if (p->x_sup && ((estep_mode != SBCE_ESTEP_SOFT && estep_mode != SBCE_ESTEP_HARD) ||
                         !aligned16(p->x_sup)))
            return SBCE_EINVAL;
        if (nz && (rc = check_noise(p, nz, pb))) return rc;
        if (cv && (rc = check_conv(p, cv, pb))) return rc;
        bool prior;
        if ((rc = check_prior(p, pr_, estep_mode, &prior))) return rc;
        if (prior && cv && cv->ll_hist) return SBCE_EUNSUPPORTED;   // sbce_loglik has no prior
        pr = prior ? pr_ : nullptr;
        empty = pb.B == 0 || iters == 0;
        c = carve(pb, solve_mode);
        ws = (char*)p->workspace;
        done = (int32_t*)(ws + c.done);
        early = p->h_true != nullptr;
        // L <= 64: the whole M-step in one launch (BASELINE cfg 5: L = 32)
        small = mstep_small_supported(pb, solve_mode) && !(gauss && pb.NR == 1);
        // n_tx <= 2 small path: its solve launch zeroes the E-step's list counters for the next
        // iteration, em_init_kernel for the first -- no counter memset per E-step
        small2 = small && mstep_small2_selected(pb);
        list_cnt = c.has_prep ? (int32_t*)(ws + c.list) + (size_t)pb.B * pb.Td : nullptr;
        // The fixed-point freeze: the plain chain is a pure function of theta
        // per trial, so once the back substitution stores the theta it overwrites bit for bit, the
        // trial's later iterations would repeat this one -- the back substitution flags the trial
        // and the kernels skip it.  Armed only where theta is the whole state and nothing reads it
        // per iteration: not with the noise estimate, the conv stop (it owns the flags), the oracle
        // stop (iters_done counts executed iterations), the LLF history or superimposed pilots, and
        // only on the batched-panel solve, whose back substitutions carry the fold.
        freeze = !nz && !cv && !early && !p->llf && !p->x_sup && !small &&
                 chol_batched_selected(pb, solve_mode);
        // The moment-repeat rule: the M-step is a pure function of the moments
        // and the call's constant inputs, so a trial whose E-step rewrote its moments bit for bit
        // is at its fixed point one M-step before the theta compare sees it.  The moment stores of
        // the E-step flag a change in mchg[b]; the M-step's launches skip a trial without one and
        // the back substitution freezes it.  Armed with the freeze, and only where every moment
        // writer of the launched E-step carries the fold.
        momfreeze = freeze && estep_momfold_supported(pb, estep_mode);
        mchg = momfreeze ? (int32_t*)(ws + c.mchg) : nullptr;
        return SBCE_OK;
    }

    int begin() {
        if (empty) return SBCE_OK;
        int rc;
        if ((rc = hip_rc(launch_em_init(pb.B, done, mchg, p->status,
                                        debug_nondefault() ? SBCE_STATUS_DEBUG : 0,
                                        small2 ? list_cnt : nullptr, s, freeze ? rep : nullptr, rep_gen,
                                        rep_word))))
            return rc;

        ea = estep_args(p, ws + c.mom, ws, &c);
        ea.done = (early || cv || freeze) ? done : nullptr;
        if (pr) {                            // constant within the call: the chain stays a pure
            ea.la = pr->la;                  // function of theta per trial
            ea.labels = pr->labels;
        }
        if (nz) {                            // the estimate starts at the caller's parameter
            if ((rc = hip_rc(launch_noise_init(pb.B, nz->varn_est, p->varn_t, pb.varn, s))))
                return rc;
            ea.varn_t = nz->varn_est;
        }
        ea.lists_zeroed = small2 && list_cnt != nullptr;
        ma = mstep_args(pb, p, ea.mom, ws, c, solve_mode);
        ma.done = ea.done;
        if (freeze) ma.freeze_w = done;
        if (momfreeze) ma.mchg = mchg;
        if (freeze) ma.report = rep;

        eas = ea;                            // superimposed pilots: E-step on y - H x_p
        if (p->x_sup) eas.yd = (const cd*)(ws + c.ysh);
        // the Kronecker factors of the pilot regressors do not change across iterations
        prefactor = rbuild_herm_supported(pb);
        if (prefactor && (rc = hip_rc(launch_pilot_factor(pb, ma, s)))) return rc;
        // the LLF kernel reads theta before the stop decision of the same iteration: no fold with
        // it nor with the noise update, which follows a trial's last M-step
        fold_stop = small2 && early && !p->llf && !nz;
        if (cv) {                            // theta_{-1} is the caller's h_initial
            char* cs = (char*)cv->scratch;
            double* ll_cur = (double*)(cs + conv_prev_bytes(pb));
            ca.theta = ma.theta; ca.prev = (cd*)cs; ca.ll_cur = ll_cur;
            ca.dth_hist = cv->dtheta_hist; ca.ll_hist = cv->ll_hist; ca.done = done;
            ca.iters_done = p->iters_done; ca.status = p->status;
            ca.tol_theta2 = cv->tol_theta * cv->tol_theta; ca.tol_ll = cv->tol_ll;
            ca.min_iters = cv->min_iters; ca.iters = iters;
            if (cv->ll_hist) {
                la = loglik_args(pb, p, ll_cur, nullptr, cs + conv_prev_bytes(pb) + conv_ll_bytes(pb));
                la.varn_t = ea.varn_t;       // the current parameter (the estimate, with nz)
                la.done = done;
            }
            if ((rc = hip_rc(launch_conv_init(pb, ma.theta, ca.prev, s)))) return rc;
        }
        return SBCE_OK;
    }

    int iteration(int it) {
        if (empty) return SBCE_OK;
        int rc;
        if (p->x_sup) {
            if ((rc = hip_rc(launch_sup_shift_y(pb, ea.yd, ea.psid, ea.theta, (const cd*)p->x_sup,
                                                (cd*)(ws + c.ysh), ea.done, s))))
                return rc;
            if ((rc = hip_rc(launch_estep(pb, eas, estep_mode, s)))) return rc;
            if ((rc = hip_rc(launch_sup_shift_mom(pb, ea.mom, (const cd*)p->x_sup, ea.done, s))))
                return rc;
        } else {
            // iteration 0: mom holds stale contents -- nothing to compare with, every trial changed
            ea.mchg = (momfreeze && it > 0) ? mchg : nullptr;
            if ((rc = hip_rc(launch_estep(pb, ea, estep_mode, s)))) return rc;
        }
        if (small) {
            MstepArgs ms = ma;
            if (ea.lists_zeroed) ms.zero_cnt = list_cnt;
            if (fold_stop) {                 // the oracle early stop rides in the M-step launch
                ms.h_true = (const cd*)p->h_true;
                ms.done_w = done;
                ms.iters_done = p->iters_done;
                ms.it = it;
            }
            if ((rc = hip_rc(launch_mstep_small(pb, ms, false, s)))) return rc;
        } else {
            if (momfreeze && it > 0) ma.mskip = mchg;
            if ((rc = hip_rc(launch_mstep_build(pb, ma, s, prefactor)))) return rc;
            // Gaussian prior, n_rx = 1: the reference's all-ones covariance term stays in A
            // (MIMO_Gaussian_proposed.py:73-76): R += c 1 1^T
            if (gauss && pb.NR == 1 && (rc = hip_rc(launch_gauss_rank1(pb, ma, s)))) return rc;
            if ((rc = hip_rc(launch_chol_solve(pb, ma, s)))) return rc;
        }
        if (p->llf &&
            (rc = hip_rc(launch_llf(pb, ma.theta, ma.yp, ma.up, ma.yd, ma.psid,
                                    (const cd*)p->x_d_true, p->llf, iters, it, ea.done, p->varn_t,
                                    s))))
            return rc;
        if (nz && (rc = noise_update(pb, p, ea.mom, ea.done, nz, nullptr, iters, it, s))) return rc;
        if (early && !fold_stop &&
            (rc = hip_rc(launch_early_stop(pb, ma.theta, (const cd*)p->h_true, done, p->iters_done,
                                           it, s))))
            return rc;
        if (cv) {
            if (cv->ll_hist && (rc = hip_rc(launch_loglik(pb, la, s)))) return rc;
            ca.it = it;
            if ((rc = hip_rc(launch_conv_step(pb, ca, s)))) return rc;
        }
        return SBCE_OK;
    }

    int finish() {
        if (empty) return SBCE_OK;
        int rc;
        if (p->x_dest && (rc = hip_rc(launch_decisions(pb, ea.mom, (cd*)p->x_dest, s)))) return rc;
        if (!early && !cv && p->iters_done) {
            // every trial ran all iterations: fill with `iters` via a tiny host-free memset pattern
            // (int32 fill is done on device by hipMemsetD32Async)
            if (hipMemsetD32Async((hipDeviceptr_t)p->iters_done, iters, (size_t)pb.B, s) != hipSuccess)
                return SBCE_EHIP;
        }
        return SBCE_OK;
    }
};

int em_run(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
           const sbce_noise_opts* nz, const sbce_conv_opts* cv, void* hip_stream,
           const sbce_prior_opts* pr = nullptr) {
    clear_stale_error();
    EmChain ch;
    int rc = ch.check(d, p, iters, estep_mode, solve_mode, nz, cv, hip_stream, pr);
    if (rc) return rc;
    if ((rc = ch.begin())) return rc;
    for (int it = 0; it < iters; ++it)
        if ((rc = ch.iteration(it))) return rc;
    return ch.finish();
}

// ---- sbce_em_multi's pacing: what a paced problem needs from the library, pooled.
// A slot holds one int32 of pinned, host-mapped, coherent memory (the word the device stores the
// call's generation to), the device counter of frozen trials and the events of the iterations in
// flight.  Slots are made on first need, kept for the life of the process and handed out under a
// mutex: a steady-state call allocates nothing.  The word is never reset: every call compares
// with a generation of its own, so what an earlier call stored compares unequal.
constexpr int kMultiMax = 8;
#ifndef SBCE_EM_LEAD_DEFAULT
#define SBCE_EM_LEAD_DEFAULT 2
#endif
// The default lead and the wait (0: hipEventSynchronize on blocking-sync events, 1: a spin on
// hipEventQuery) were chosen by measurement at cfg1 (profiles/emstop/README.md: leads 1 / 2 / 3
// and both waits as arms built with these macros); the two waits do not differ there, and the
// blocking one leaves the host core free.
#ifndef SBCE_EM_WAIT_SPIN
#define SBCE_EM_WAIT_SPIN 0
#endif

struct PaceSlot {
    int device = -1;
    bool busy = false;
    int32_t* word = nullptr;       // host address
    int32_t* word_dev = nullptr;   // the same word as the device sees it
    FreezeReport* rep = nullptr;   // device memory: the counter, the generation, the word's address
    std::vector<hipEvent_t> ev;    // ring of `lead` events, grown to the largest lead seen
    hipEvent_t tail = nullptr;     // end of the last call that used the slot
    hipStream_t last = nullptr;    // ... and its stream
    bool used = false;
};

std::mutex g_pace_mu;
std::vector<PaceSlot*> g_pace;
std::atomic<uint32_t> g_pace_gen{0};

constexpr unsigned kPaceEventFlags =
    hipEventDisableTiming | (SBCE_EM_WAIT_SPIN ? 0u : (unsigned)hipEventBlockingSync);

void pace_release(PaceSlot* sl) {
    std::lock_guard<std::mutex> lk(g_pace_mu);
    sl->busy = false;
}

// A free slot of `device` with at least `nev` events, preferring the one this stream used last
// (its counter and word are then ordered by the stream itself).  A slot last used on another
// stream may still have that call's tail in flight: the new stream waits for its end first, so
// the counter is never zeroed under a late increment.
int pace_acquire(int device, hipStream_t s, int nev, PaceSlot** out) {
    PaceSlot* sl = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pace_mu);
        for (PaceSlot* q : g_pace) {
            if (q->busy || q->device != device) continue;
            if (!sl || (q->used && q->last == s)) sl = q;
            if (sl->used && sl->last == s) break;
        }
        if (!sl) {
            sl = new PaceSlot;
            sl->device = device;
            g_pace.push_back(sl);
        }
        sl->busy = true;
    }
    // each resource is made where it is still missing, so a slot whose first set-up failed half
    // way is completed by the next call instead of being used half-built
    bool ok = true;
    if (!sl->word) {
        void* h = nullptr;
        ok = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
        if (ok) {
            sl->word = (int32_t*)h;
            *sl->word = 0;
        }
    }
    if (ok && !sl->word_dev) {
        void* dv = nullptr;
        ok = hipHostGetDevicePointer(&dv, sl->word, 0) == hipSuccess && dv;
        if (ok) sl->word_dev = (int32_t*)dv;
    }
    if (ok && !sl->rep) {
        void* r = nullptr;
        ok = hipMalloc(&r, sizeof(FreezeReport)) == hipSuccess && r;
        if (ok) sl->rep = (FreezeReport*)r;
    }
    if (ok && !sl->tail) {
        hipEvent_t e = nullptr;
        ok = hipEventCreateWithFlags(&e, kPaceEventFlags) == hipSuccess;
        if (ok) sl->tail = e;
    }
    while (ok && (int)sl->ev.size() < nev) {
        hipEvent_t e;
        ok = hipEventCreateWithFlags(&e, kPaceEventFlags) == hipSuccess;
        if (ok) sl->ev.push_back(e);
    }
    if (ok && sl->used && sl->last != s) ok = hipStreamWaitEvent(s, sl->tail, 0) == hipSuccess;
    if (!ok) {
        pace_release(sl);
        return SBCE_EHIP;
    }
    *out = sl;
    return SBCE_OK;
}

// The host waits only for work that is already enqueued, never for the word itself.
int pace_wait(hipEvent_t e) {
#if SBCE_EM_WAIT_SPIN
    hipError_t r;
    while ((r = hipEventQuery(e)) == hipErrorNotReady) {
    }
    (void)hipGetLastError();                 // "not ready" is no error of this call's launches
    return hip_rc(r);
#else
    return hip_rc(hipEventSynchronize(e));
#endif
}

}  // namespace

extern "C" {

int sbce_em(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
            void* hip_stream) {
    return em_run(d, p, iters, estep_mode, solve_mode, nullptr, nullptr, hip_stream);
}

int sbce_em_noise(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
                  const sbce_noise_opts* o, void* hip_stream) {
    if (!o) return SBCE_EINVAL;
    return em_run(d, p, iters, estep_mode, solve_mode, o, nullptr, hip_stream);
}

int sbce_em_multi(int n, const sbce_dims* const* dims, const sbce_ptrs* const* ptrs, int iters,
                  int estep_mode, int solve_mode, void* const* hip_streams, int lead,
                  int* iters_issued) {
    if (n < 1 || n > kMultiMax || !dims || !ptrs || !hip_streams) return SBCE_EINVAL;
    if (lead < 0 || (lead > 0 && lead > iters)) return SBCE_EINVAL;
    EmChain ch[kMultiMax];
    for (int j = 0; j < n; ++j) {            // every argument, before any HIP call
        const int rc = ch[j].check(dims[j], ptrs[j], iters, estep_mode, solve_mode, nullptr, nullptr,
                                   hip_streams[j]);
        if (rc) return rc;
    }
    if (lead == 0) lead = SBCE_EM_LEAD_DEFAULT < iters ? SBCE_EM_LEAD_DEFAULT : iters;
    clear_stale_error();
    PaceSlot* slot[kMultiMax] = {};
    int issued[kMultiMax] = {};
    bool ended[kMultiMax] = {};
    int rc = SBCE_OK;
    // a problem is paced where its freeze is armed and its stream is not capturing (a capture
    // records the whole fixed launch sequence; an event wait has no place in it)
    int device = 0;
    for (int j = 0; j < n && !rc; ++j) {
        EmChain& c = ch[j];
        if (!c.freeze || c.empty || lead >= iters) continue;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c.s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            continue;
        }
        if (hipGetDevice(&device) != hipSuccess) { rc = SBCE_EHIP; break; }
        if ((rc = pace_acquire(device, c.s, lead, &slot[j]))) break;
        uint32_t g = ++g_pace_gen;
        if (g == 0) g = ++g_pace_gen;        // the generation is never zero
        c.rep = slot[j]->rep;
        c.rep_word = slot[j]->word_dev;
        c.rep_gen = (int32_t)g;
    }
    for (int j = 0; j < n && !rc; ++j) rc = ch[j].begin();
    for (int it = 0; it < iters && !rc; ++it) {
        for (int j = 0; j < n && !rc; ++j) {
            if (ended[j]) continue;
            PaceSlot* sl = slot[j];
            if (sl && it >= lead) {
                // iteration it - lead is complete: if it (or an earlier one) froze the last live
                // trial, the word holds this call's generation and every later iteration is the
                // identity -- none is issued
                if ((rc = pace_wait(sl->ev[it % lead]))) break;
                if (__atomic_load_n(sl->word, __ATOMIC_ACQUIRE) == ch[j].rep_gen) {
                    ended[j] = true;
                    continue;
                }
            }
            if ((rc = ch[j].iteration(it))) break;
            if (!ch[j].empty) ++issued[j];
            if (sl && it + lead < iters) rc = hip_rc(hipEventRecord(sl->ev[it % lead], ch[j].s));
        }
    }
    for (int j = 0; j < n; ++j) {
        if (!rc) rc = ch[j].finish();
        if (slot[j]) {
            if (hipEventRecord(slot[j]->tail, ch[j].s) == hipSuccess) {
                slot[j]->last = ch[j].s;
                slot[j]->used = true;
            } else if (!rc) {
                rc = SBCE_EHIP;
            }
            pace_release(slot[j]);
        }
        if (iters_issued) iters_issued[j] = issued[j];
    }
    return rc;
}

int sbce_conv_workspace_bytes(const sbce_dims* d, int want_ll, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb)) return SBCE_EINVAL;
    *bytes = conv_scratch_bytes(pb, want_ll != 0);
    return SBCE_OK;
}

int sbce_em_conv(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
                 const sbce_noise_opts* nz, const sbce_conv_opts* cv, void* hip_stream) {
    if (!cv) return SBCE_EINVAL;
    return em_run(d, p, iters, estep_mode, solve_mode, nz, cv, hip_stream);
}

int sbce_em_prior(const sbce_dims* d, const sbce_ptrs* p, int iters, int estep_mode, int solve_mode,
                  const sbce_prior_opts* pr, const sbce_noise_opts* nz, const sbce_conv_opts* cv,
                  void* hip_stream) {
    return em_run(d, p, iters, estep_mode, solve_mode, nz, cv, hip_stream, pr);
}

int sbce_loglik_workspace_bytes(const sbce_dims* d, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb)) return SBCE_EINVAL;
    *bytes = loglik_scratch_bytes(pb);
    return SBCE_OK;
}

int sbce_loglik(const sbce_dims* d, const sbce_ptrs* p, double* ll, double* ll_sym, void* scratch,
                size_t scratch_bytes, void* hip_stream) {
    Problem pb;
    if (!make_problem(d, pb)) return SBCE_EINVAL;
    int rc = check_ptrs(p, pb, false);
    if (rc) return rc;
    if (p->x_sup) return SBCE_EINVAL;
    if (!ll || ((uintptr_t)ll & 7) || ((uintptr_t)ll_sym & 7)) return SBCE_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 7)) return SBCE_EINVAL;
    if (!loglik_supported(pb)) return SBCE_EUNSUPPORTED;
    if (scratch_bytes < loglik_scratch_bytes(pb)) return SBCE_EWORKSPACE;
    if (pb.B == 0) return SBCE_OK;
    clear_stale_error();
    return hip_rc(launch_loglik(pb, loglik_args(pb, p, ll, ll_sym, (char*)scratch),
                                (hipStream_t)hip_stream));
}

int sbce_noise_workspace_bytes(const sbce_dims* d, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb)) return SBCE_EINVAL;
    *bytes = noise_scratch_bytes(pb);
    return SBCE_OK;
}

int sbce_noise_var(const sbce_dims* d, const sbce_ptrs* p, const void* moments,
                   const sbce_noise_opts* o, void* hip_stream) {
    Problem pb;
    if (!make_problem(d, pb) || !p || !o) return SBCE_EINVAL;
    if (!required({p->y_d, p->y_p, p->psi_d, p->u_p, p->theta, moments})) return SBCE_EINVAL;
    if (p->varn_t && ((uintptr_t)p->varn_t & 7)) return SBCE_EINVAL;
    if (int rc = check_noise(p, o, pb)) return rc;
    if (pb.B == 0) return SBCE_OK;
    clear_stale_error();
    NoiseFinalArgs f{};
    f.prev_t = p->varn_t; f.prev = pb.varn;
    f.status_base = debug_nondefault() ? SBCE_STATUS_DEBUG : 0;
    return noise_update(pb, p, (const cd*)moments, nullptr, o, &f, 1, 0, (hipStream_t)hip_stream);
}

int sbce_estep(const sbce_dims* d, const sbce_ptrs* p, int estep_mode, void* moments,
               void* hip_stream) {
    return sbce_estep_prior(d, p, estep_mode, nullptr, moments, hip_stream);
}

int sbce_estep_prior(const sbce_dims* d, const sbce_ptrs* p, int estep_mode,
                     const sbce_prior_opts* pr, void* moments, void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (linear_oversize(d, estep_mode)) return SBCE_EUNSUPPORTED;
    if (!make_problem(d, pb)) return SBCE_EINVAL;
    if (ep_passes_invalid(pb, estep_mode)) return SBCE_EINVAL;
    int rc = check_ptrs(p, pb, false);
    if (rc) return rc;
    if (!moments || !aligned16(moments)) return SBCE_EINVAL;
    if (estep_mode == SBCE_ESTEP_GAUSS && !(pb.varx > 0.0)) return SBCE_EINVAL;
    if (!estep_supported(pb, estep_mode)) return SBCE_EUNSUPPORTED;
    bool prior;
    if ((rc = check_prior(p, pr, estep_mode, &prior))) return rc;
    if (pb.B == 0) return SBCE_OK;
    if ((rc = status_init(p->status, pb.B, (hipStream_t)hip_stream))) return rc;
    // workspace optional here: use it when it is large enough (the E-step regions come first)
    const Carve c = carve(pb, SBCE_SOLVE_CHOL);
    const bool use_ws = p->workspace && aligned16(p->workspace) && p->workspace_bytes >= c.total;
    EstepArgs ea = estep_args(p, moments, (char*)p->workspace, use_ws ? &c : nullptr);
    if (prior) {
        ea.la = pr->la;
        ea.labels = pr->labels;
    }
    return hip_rc(launch_estep(pb, ea, estep_mode, (hipStream_t)hip_stream));
}

int sbce_mstep(const sbce_dims* d, const sbce_ptrs* p, const void* moments, int solve_mode,
               void* r_out, void* rhs_out, void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb)) return SBCE_EINVAL;
    if (!chol_supported(pb)) return SBCE_EUNSUPPORTED;
    if (!valid_solve(solve_mode)) return SBCE_EINVAL;
    int rc = check_ptrs(p, pb, true, solve_mode);
    if (rc) return rc;
    if (!moments) return SBCE_EINVAL;
    if (pb.B == 0) return SBCE_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const Carve c = carve(pb, solve_mode);
    char* ws = (char*)p->workspace;
    if ((rc = status_init(p->status, pb.B, s))) return rc;
    const MstepArgs ma = mstep_args(pb, p, moments, ws, c, solve_mode);
    const bool small = mstep_small_supported(pb, solve_mode);
    if (small) {
        if ((rc = hip_rc(launch_mstep_small(pb, ma, r_out || rhs_out, s)))) return rc;
    } else if ((rc = hip_rc(launch_mstep_build(pb, ma, s)))) {
        return rc;
    }
    if (r_out &&
        hipMemcpyAsync(r_out, ma.R, (size_t)pb.B * pb.L * pb.L * sizeof(cd), hipMemcpyDeviceToDevice,
                       s) != hipSuccess)
        return SBCE_EHIP;
    if (rhs_out &&
        hipMemcpyAsync(rhs_out, ma.rhs, (size_t)pb.B * pb.L * pb.NR * sizeof(cd),
                       hipMemcpyDeviceToDevice, s) != hipSuccess)
        return SBCE_EHIP;
    return small ? SBCE_OK : hip_rc(launch_chol_solve(pb, ma, s));
}

int sbce_crb_workspace_bytes(const sbce_dims* d, size_t* bytes) {
    Problem pb;
    if (!bytes || !make_problem(d, pb)) return SBCE_EINVAL;
    if (!chol_supported(pb) || pb.L > kLargeL) return SBCE_EUNSUPPORTED;
    *bytes = crb_scratch_bytes(pb);
    return SBCE_OK;
}

int sbce_crb(const sbce_dims* d, const sbce_ptrs* p, const void* moments, const sbce_crb_opts* o,
             void* hip_stream) {
    Problem pb;
    if (!make_problem(d, pb)) return SBCE_EINVAL;
    if (!chol_supported(pb) || pb.L > kLargeL) return SBCE_EUNSUPPORTED;
    int rc = check_ptrs(p, pb, true, SBCE_SOLVE_CHOL);
    if (rc) return rc;
    if (!moments) return SBCE_EINVAL;
    if (!o || !o->tr_inv || !o->scratch || !aligned16(o->scratch)) return SBCE_EINVAL;
    if (((uintptr_t)o->tr_inv | (uintptr_t)o->diag_inv | (uintptr_t)o->mse | (uintptr_t)o->bound |
         (uintptr_t)o->sigma2_t) & 7)
        return SBCE_EINVAL;
    if (!(o->sigma2 > 0.0) || o->flags != 0) return SBCE_EINVAL;
    if (o->bound && (!p->h_true || !aligned16(p->h_true))) return SBCE_EINVAL;
    if (o->scratch_bytes < crb_scratch_bytes(pb)) return SBCE_EWORKSPACE;
    if (pb.B == 0) return SBCE_OK;
    clear_stale_error();
    hipStream_t s = (hipStream_t)hip_stream;
    const Carve c = carve(pb, SBCE_SOLVE_CHOL);
    char* ws = (char*)p->workspace;
    if ((rc = status_init(p->status, pb.B, s))) return rc;
    // the build of sbce_mstep; at small L it comes with the solve, whose theta goes to the scratch
    // and whose own pivot flag is not taken (the factorisation below decides)
    MstepArgs ma = mstep_args(pb, p, moments, ws, c, SBCE_SOLVE_CHOL);
    char* sc = (char*)o->scratch;
    if (mstep_small_supported(pb, SBCE_SOLVE_CHOL)) {
        ma.theta = (cd*)(sc + align_up(crb_dinv_bytes(pb)));
        ma.status = nullptr;
        if ((rc = hip_rc(launch_mstep_small(pb, ma, true, s)))) return rc;
    } else if ((rc = hip_rc(launch_mstep_build(pb, ma, s)))) {
        return rc;
    }
    return hip_rc(launch_crb(pb, ma.R, (cd*)sc, (const cd*)p->h_true, *o, p->status, s));
}

// Diagnostic, not part of include/sbce.h: HIP-event timing of the L <= 512 Cholesky's update /
// factor / back-substitution launches (bench.py's panel_factor line).  mode 1 arms it for the
// following M-steps; mode 0 (after the caller synchronised) returns {update, factor, back
// substitution} ms and launch counts in out6 and disarms it.
int sbce_debug_chol_timing(int mode, double* out6) {
    clear_stale_error();
    return hip_rc(chol_debug_timing(mode, out6));
}

// Diagnostic, not part of include/sbce.h: per-phase cycle sums (32) of the MFMA Cholesky
// (SBCE_CHOL_SKIP bit 64); reset != 0 clears them.
// Diagnostic, not part of include/sbce.h: s_memtime stamps (48) of trial 0's solve wave in the
// n_tx <= 2 small M-step (SBCE_SMALL_STOP=4).
int sbce_debug_small_clock(unsigned long long* out48) {
    return out48 ? hip_rc(small_debug_clock(out48)) : SBCE_EINVAL;
}

int sbce_debug_chol_clock(unsigned long long* out32, int reset) {
    if (reset) return hip_rc(chol_debug_clock_reset());
    return out32 ? hip_rc(chol_debug_clock(out32)) : SBCE_EINVAL;
}

// Diagnostic, not part of include/sbce.h: phase-skip mask of the L <= 512 Cholesky kernels (1
// panel update, 2 diagonal factor, 8 TRSM tiles, 16 back substitution: results INVALID; 64:
// per-phase clocks of the fused kernel, results valid).  Process-wide (every thread and
// stream); while bits 0-4 are set every trial of every path is flagged SBCE_STATUS_DEBUG.
// 0 restores normal operation.
int sbce_debug_chol_skip(int mask) {
#if SBCE_AB
    if (mask < 0) return SBCE_EINVAL;
    chol_debug_skip(mask);
    return SBCE_OK;
#else
    (void)mask;
    return SBCE_EUNSUPPORTED;                        // libsbce_ab.so only
#endif
}

// Diagnostic, not part of include/sbce.h: the decoder kernel as one wave per codeword group
// (alpha over every step, then beta with the outputs) instead of the two-wave split, for the A/B
// timing of tools/siso_bench.py; the results are bitwise the same.
int sbce_debug_siso_onewave(int on) {
#if SBCE_AB
    siso_debug_onewave(on);
    return SBCE_OK;
#else
    (void)on;
    return SBCE_EUNSUPPORTED;                        // libsbce_ab.so only
#endif
}

// Diagnostic, not part of include/sbce.h: one piece of the M-step for kernel timing (bench.py's
// dominant-kernel roofline), from the given moments: phase 0 = the pilot factorisation (once per
// EM run), 1 = the R build alone (the MFMA Hermitian build rbuild_herm_kernel when n_tx is 4 or
// 8 -- phase 0 must have run -- else the VALU build with B^H), 2 = the whole build (R and B^H).
int sbce_debug_mstep_phase(const sbce_dims* d, const sbce_ptrs* p, const void* moments, int phase,
                           void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb)) return SBCE_EINVAL;
    if (!chol_supported(pb)) return SBCE_EUNSUPPORTED;
    int rc = check_ptrs(p, pb, true, SBCE_SOLVE_CHOL);
    if (rc) return rc;
    if (!moments || phase < 0 || phase > 2) return SBCE_EINVAL;
    if (pb.B == 0) return SBCE_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const Carve c = carve(pb, SBCE_SOLVE_CHOL);
    char* ws = (char*)p->workspace;
    MstepArgs ma = mstep_args(pb, p, moments, ws, c, SBCE_SOLVE_CHOL);
    ma.status = nullptr;
    if (phase == 0) return rbuild_herm_supported(pb) ? hip_rc(launch_pilot_factor(pb, ma, s)) : SBCE_OK;
    if (phase == 1 && rbuild_herm_supported(pb)) return hip_rc(launch_rbuild_herm(pb, ma, s));
    return hip_rc(launch_mstep_build(pb, ma, s, rbuild_herm_supported(pb)));
}

// Diagnostic, not part of include/sbce.h: the per-trial pivot threshold tau = 32 eps K lambda_max
// the last min-norm M-step left in the workspace (tol_out [B] doubles, host or device memory).
int sbce_debug_minnorm_tol(const sbce_dims* d, const sbce_ptrs* p, double* tol_out, void* hip_stream) {
    Problem pb;
    if (!make_problem(d, pb) || !tol_out) return SBCE_EINVAL;
    int rc = check_ptrs(p, pb, true, SBCE_SOLVE_CHOL);
    if (rc) return rc;
    const Carve c = carve(pb, SBCE_SOLVE_CHOL);           // tol precedes the solve regions
    return hip_rc(hipMemcpyAsync(tol_out, (char*)p->workspace + c.tol, (size_t)pb.B * sizeof(double),
                                 hipMemcpyDefault, (hipStream_t)hip_stream));
}

// Diagnostic, not part of include/sbce.h: per trial (active extent, rank, refinement ran) of the
// last SBCE_SOLVE_MINNORM M-step whose workspace `p` holds (out3: [B][3] int32, device memory);
// bench.py prices the min-norm solve at its executed flops from them.
int sbce_debug_minnorm_rank(const sbce_dims* d, const sbce_ptrs* p, int32_t* out3, void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb) || !out3) return SBCE_EINVAL;
    int rc = check_ptrs(p, pb, true, SBCE_SOLVE_MINNORM);
    if (rc) return rc;
    if (pb.B == 0) return SBCE_OK;
    const Carve c = carve(pb, SBCE_SOLVE_MINNORM);
    MstepArgs ma;
    ma.R = (cd*)((char*)p->workspace + c.R);
    ma.done = nullptr;
    ma.nbatch = pb.B;
    set_large(ma, (char*)p->workspace, c);
    return hip_rc(launch_minnorm_rank(pb, ma, out3, (hipStream_t)hip_stream));
}

// Diagnostic, not part of include/sbce.h: re-read the SBCE_* debug switches from the
// environment (they are otherwise read once, when the library is loaded).  Returns 1 when a
// result-affecting switch is now non-default (every trial is then flagged SBCE_STATUS_DEBUG).
// The product build has no switches and reads nothing: it returns -1.
int sbce_debug_reload_env(void) {
#if SBCE_AB
    read_debug_env(g_debug);
    return debug_nondefault() ? 1 : 0;
#else
    return -1;
#endif
}

// Diagnostic, not part of include/sbce.h: FP64 MFMAs issued by the exact E-step sweep since
// the last reset (counted only with SBCE_ESTEP_COUNT=1); reset != 0 clears the counter.
int sbce_debug_estep_mfma(unsigned long long* out, int reset) {
    if (!reset && !out) return SBCE_EINVAL;
    return hip_rc(estep_debug_mfma(out, reset));
}

// Diagnostic, not part of include/sbce.h: tile groups of the V16 sweep that survived every bound
// and reached the FP32 screen (or, with the screen off, the FP64 test) since the last reset
// (counted only with SBCE_ESTEP_COUNT=1); reset != 0 clears the counter.
int sbce_debug_estep_groups(unsigned long long* out, int reset) {
    if (!reset && !out) return SBCE_EINVAL;
    return hip_rc(estep_debug_groups(out, reset));
}

// Diagnostic, not part of include/sbce.h: tile groups the second pass of the two-pass V16 soft
// sweep recomputed since the last reset (counted only with SBCE_ESTEP_COUNT=1; 8 FP64 MFMAs each,
// on top of sbce_debug_estep_mfma, which stays the search's count); reset != 0 clears the counter.
int sbce_debug_estep_pass2(unsigned long long* out, int reset) {
    if (!reset && !out) return SBCE_EINVAL;
    return hip_rc(estep_debug_pass2(out, reset));
}

// Diagnostic, not part of include/sbce.h: trial-M-steps the moment-repeat rule of sbce_em skipped
// since the last reset (every stream); reset != 0 clears the counter.  The counter exists only in
// the A/B build: the product library returns SBCE_EUNSUPPORTED.
int sbce_debug_momskip(unsigned long long* out, int reset) {
#if SBCE_AB
    if (!reset && !out) return SBCE_EINVAL;
    return hip_rc(mstep_debug_momskip(out, reset));
#else
    (void)out; (void)reset;
    return SBCE_EUNSUPPORTED;
#endif
}

// Diagnostic, not part of include/sbce.h: symbols the sphere pass resolved by enumeration
// (out3[0]), left to the MFMA sweep (out3[1]) and resolved by the tree pass's single-path check
// (out3[2]) since the last reset (counted only with SBCE_ESTEP_COUNT=1).
int sbce_debug_estep_sphere(unsigned long long* out3, int reset) {
    if (!reset && !out3) return SBCE_EINVAL;
    return hip_rc(estep_debug_sphere(out3, reset));
}

// Diagnostic, not part of include/sbce.h: listed symbols the factorised-weight pass resolved
// (estep_pair.hip) since the last reset (counted only with SBCE_ESTEP_COUNT=1).
int sbce_debug_estep_pair(unsigned long long* out, int reset) {
    if (!reset && !out) return SBCE_EINVAL;
    return hip_rc(estep_debug_pair(out, reset));
}

int sbce_ser(const sbce_dims* d, const void* x_dest, const void* x_d_true, double* ser_out,
             void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb) || !x_dest || !x_d_true || !ser_out) return SBCE_EINVAL;
    if (pb.B == 0) return SBCE_OK;
    return hip_rc(launch_ser(pb, (const cd*)x_dest, (const cd*)x_d_true, ser_out,
                             (hipStream_t)hip_stream));
}

int sbce_gauss_expand(const sbce_dims* d, const void* theta, void* h_out, void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb) || !theta || !h_out || !aligned16(theta) || !aligned16(h_out))
        return SBCE_EINVAL;
    if (pb.B == 0) return SBCE_OK;
    return hip_rc(launch_gauss_expand(pb, (const cd*)theta, (cd*)h_out, (hipStream_t)hip_stream));
}

int sbce_nmse(const sbce_dims* d, const void* theta, const void* h_true, double* nmse_out,
              void* hip_stream) {
    clear_stale_error();
    Problem pb;
    if (!make_problem(d, pb) || !theta || !h_true || !nmse_out) return SBCE_EINVAL;
    if (pb.B == 0) return SBCE_OK;
    return hip_rc(launch_nmse(pb, (const cd*)theta, (const cd*)h_true, nmse_out,
                              (hipStream_t)hip_stream));
}

int sbce_approx_workspace_bytes(const sbce_approx_dims* d, size_t* bytes) {
    if (!d || !bytes) return SBCE_EINVAL;
    *bytes = 0;                          // a trial's state lives in LDS and registers
    return SBCE_OK;
}

int sbce_approx_em(const sbce_approx_dims* d, const sbce_approx_ptrs* p, int iters,
                   void* hip_stream) {
    if (!d || !p) return SBCE_EINVAL;
    if (d->batch < 1 || d->n_ris < 1 || d->n_rx < 1 || d->t_p < 1 || d->t_d < 1 || iters < 1 ||
        !(d->varn > 0.0))
        return SBCE_EINVAL;
    if (!required({p->y_d, p->y_p, p->psi_d, p->psi_p, p->x_p, p->g})) return SBCE_EINVAL;
    if (p->varn_t && ((uintptr_t)p->varn_t & 7)) return SBCE_EINVAL;
    if (!approx_supported(d->n_ris, d->n_rx)) return SBCE_EUNSUPPORTED;
    clear_stale_error();
    ApproxArgs a;
    a.yd = (const cd*)p->y_d; a.yp = (const cd*)p->y_p; a.psid = (const cd*)p->psi_d;
    a.psip = (const cd*)p->psi_p; a.xp = (const cd*)p->x_p; a.g = (cd*)p->g;
    a.varn_t = p->varn_t; a.status = p->status;
    a.B = d->batch; a.N = d->n_ris; a.M = d->n_rx; a.Tp = d->t_p; a.Td = d->t_d; a.iters = iters;
    a.varn = d->varn;
    a.status0 = debug_nondefault() ? SBCE_STATUS_DEBUG : 0;
    return hip_rc(launch_approx(a, (hipStream_t)hip_stream));
}

int sbce_detect_workspace_bytes(const sbce_detect_dims* d, size_t* bytes) {
    if (!d || !bytes) return SBCE_EINVAL;
    *bytes = 0;                          // a symbol's state lives in LDS and registers
    return SBCE_OK;
}

int sbce_detect(const sbce_detect_dims* d, const sbce_detect_ptrs* p, void* hip_stream) {
    if (!d || !p) return SBCE_EINVAL;
    if (d->batch < 1 || d->n_tx < 1 || d->n_rx < 1 || d->n_psi < 1 || d->t_d < 1 ||
        !(d->sigma2 > 0.0) || (d->flags & ~SBCE_DETECT_MAXLOG))
        return SBCE_EINVAL;
    if (d->m < 2 || d->m > 64 || (d->m & (d->m - 1))) return SBCE_EINVAL;   // a power of two
    if (!required({p->y_d, p->psi_d, p->cons, p->theta})) return SBCE_EINVAL;
    if ((p->llr || p->err) && !p->labels) return SBCE_EINVAL;
    if (p->err && !p->x_d_true) return SBCE_EINVAL;
    if (!aligned16(p->x_d_true) || !aligned16(p->x_hat)) return SBCE_EINVAL;
    if (((uintptr_t)p->sigma2_t & 7) || ((uintptr_t)p->post & 7) || ((uintptr_t)p->llr & 7))
        return SBCE_EINVAL;
    if (((uintptr_t)p->labels & 3) || ((uintptr_t)p->idx_hat & 3) || ((uintptr_t)p->err & 3))
        return SBCE_EINVAL;
    if (!detect_supported(d->n_tx, d->n_rx, d->m)) return SBCE_EUNSUPPORTED;
    size_t need = 0;
    sbce_detect_workspace_bytes(d, &need);
    if (need && (!p->workspace || !aligned16(p->workspace))) return SBCE_EINVAL;
    if (p->workspace_bytes < need) return SBCE_EWORKSPACE;
    clear_stale_error();
    DetectArgs a{};                      // lgM, TC and chunks are launch_detect's
    a.yd = (const cd*)p->y_d; a.psid = (const cd*)p->psi_d; a.cons = (const cd*)p->cons;
    a.theta = (const cd*)p->theta; a.labels = p->labels; a.sigma2_t = p->sigma2_t;
    a.xd = (const cd*)p->x_d_true; a.xhat = (cd*)p->x_hat; a.idx = p->idx_hat; a.post = p->post;
    a.llr = p->llr; a.err = p->err;
    a.B = d->batch; a.NT = d->n_tx; a.NR = d->n_rx; a.P = d->n_psi; a.Td = d->t_d; a.M = d->m;
    a.maxlog = (d->flags & SBCE_DETECT_MAXLOG) ? 1 : 0;
    a.sigma2 = d->sigma2;
    return hip_rc(launch_detect(a, (hipStream_t)hip_stream));
}

int sbce_detect_linear_workspace_bytes(const sbce_linear_dims* d, size_t* bytes) {
    if (!d || !bytes) return SBCE_EINVAL;
    *bytes = 0;                          // a symbol's state lives in LDS and registers
    return SBCE_OK;
}

int sbce_detect_linear(const sbce_linear_dims* d, const sbce_linear_ptrs* p, void* hip_stream) {
    return sbce_detect_linear_prior(d, p, nullptr, hip_stream);
}

int sbce_detect_linear_prior(const sbce_linear_dims* d, const sbce_linear_ptrs* p, const double* la,
                             void* hip_stream) {
    if (!d || !p) return SBCE_EINVAL;
    if (d->batch < 1 || d->n_tx < 1 || d->n_rx < 1 || d->n_psi < 1 || d->t_d < 1 ||
        !(d->sigma2 > 0.0))
        return SBCE_EINVAL;
    if (d->kind != SBCE_LINEAR_MMSE && d->kind != SBCE_LINEAR_ZF && d->kind != SBCE_LINEAR_EP)
        return SBCE_EINVAL;
    // flags bits 8..15 carry the EP pass count (0: the default, 1..16); unknown bits for MMSE / ZF
    const int known = SBCE_DETECT_MAXLOG | (d->kind == SBCE_LINEAR_EP ? 0xff00 : 0);
    if (d->flags & ~known) return SBCE_EINVAL;
    const int ep_word = (d->flags >> 8) & 0xff;
    if (d->kind == SBCE_LINEAR_EP && ep_passes_of(ep_word) < 0) return SBCE_EINVAL;
    if (d->kind != SBCE_LINEAR_ZF && !(d->es > 0.0)) return SBCE_EINVAL;
    if (d->m < 2 || d->m > 64 || (d->m & (d->m - 1))) return SBCE_EINVAL;   // a power of two
    if (!required({p->y_d, p->psi_d, p->cons, p->theta})) return SBCE_EINVAL;
    if ((p->llr || p->err) && !p->labels) return SBCE_EINVAL;
    if (p->err && !p->x_d_true) return SBCE_EINVAL;
    if (!aligned16(p->x_d_true) || !aligned16(p->x_hat) || !aligned16(p->x_soft) ||
        !aligned16(p->moments))
        return SBCE_EINVAL;
    if (((uintptr_t)p->sigma2_t & 7) || ((uintptr_t)p->post & 7) || ((uintptr_t)p->llr & 7) ||
        ((uintptr_t)p->nu & 7))
        return SBCE_EINVAL;
    if (((uintptr_t)p->labels & 3) || ((uintptr_t)p->idx_hat & 3) || ((uintptr_t)p->err & 3) ||
        ((uintptr_t)p->status & 3))
        return SBCE_EINVAL;
    if (d->kind == SBCE_LINEAR_ZF && d->n_rx < d->n_tx) return SBCE_EINVAL;   // H^H H is singular
    if (!detect_linear_supported(d->n_tx, d->n_rx)) return SBCE_EUNSUPPORTED;
    size_t need = 0;
    sbce_detect_linear_workspace_bytes(d, &need);
    if (need && (!p->workspace || !aligned16(p->workspace))) return SBCE_EINVAL;
    if (p->workspace_bytes < need) return SBCE_EWORKSPACE;
    if (la) {                            // the prior's own checks, after the wrapped call's
        if (!p->labels || ((uintptr_t)la & 7)) return SBCE_EINVAL;
        if (d->kind != SBCE_LINEAR_EP) return SBCE_EUNSUPPORTED;
    }
    clear_stale_error();
    LinearArgs a{};                      // lgM and chunks are launch_detect_linear's
    a.yd = (const cd*)p->y_d; a.psid = (const cd*)p->psi_d; a.cons = (const cd*)p->cons;
    a.theta = (const cd*)p->theta; a.labels = p->labels; a.sigma2_t = p->sigma2_t;
    a.xd = (const cd*)p->x_d_true; a.xsoft = (cd*)p->x_soft; a.nu = p->nu; a.xhat = (cd*)p->x_hat;
    a.idx = p->idx_hat; a.post = p->post; a.llr = p->llr; a.err = p->err; a.mom = (cd*)p->moments;
    a.status = p->status;
    a.B = d->batch; a.NT = d->n_tx; a.NR = d->n_rx; a.P = d->n_psi; a.Td = d->t_d; a.M = d->m;
    a.kind = d->kind;
    a.maxlog = (d->flags & SBCE_DETECT_MAXLOG) ? 1 : 0;
    a.passes = ep_passes_of(ep_word);
    a.sigma2 = d->sigma2; a.es = d->es;
    return hip_rc(la ? launch_detect_linear_prior(a, la, (hipStream_t)hip_stream)
                     : launch_detect_linear(a, (hipStream_t)hip_stream));
}

// The checks of sbce_siso_dims, in the header's order; n_steps on success
static int siso_check_dims(const sbce_siso_dims* d, int* n_steps) {
    if (!d) return SBCE_EINVAL;
    if (d->batch < 1 || d->n_info < 1) return SBCE_EINVAL;
    if (d->flags & ~(SBCE_DETECT_MAXLOG | SBCE_SISO_TERMINATED)) return SBCE_EINVAL;
    if (!siso_supported(d->k, d->n)) return SBCE_EUNSUPPORTED;
    for (int j = 0; j < d->n; ++j) {
        const int g = d->gen[j];
        if (g < 0 || (g >> d->k) || !((g >> (d->k - 1)) & 1) || !(g & 1)) return SBCE_EINVAL;
    }
    const long long T = (long long)d->n_info + ((d->flags & SBCE_SISO_TERMINATED) ? d->k - 1 : 0);
    if (T > kSisoMaxSteps) return SBCE_EUNSUPPORTED;
    *n_steps = (int)T;
    return SBCE_OK;
}

int sbce_siso_workspace_bytes(const sbce_siso_dims* d, size_t* bytes) {
    if (!bytes) return SBCE_EINVAL;
    int T = 0;
    const int rc = siso_check_dims(d, &T);
    if (rc != SBCE_OK) return rc;
    *bytes = siso_ws_bytes(d->batch, d->k, T);
    return SBCE_OK;
}

int sbce_siso_decode(const sbce_siso_dims* d, const sbce_siso_ptrs* p, void* hip_stream) {
    if (!d || !p || !p->lc) return SBCE_EINVAL;
    int T = 0;
    const int rc = siso_check_dims(d, &T);
    if (rc != SBCE_OK) return rc;
    if (p->err && !p->u_true) return SBCE_EINVAL;
    if (!p->lapp_u && !p->u_hat && !p->le_c && !p->err) return SBCE_EINVAL;
    if (!p->workspace || !aligned16(p->workspace)) return SBCE_EINVAL;
    if (((uintptr_t)p->lc & 7) || ((uintptr_t)p->la_u & 7) || ((uintptr_t)p->lapp_u & 7) ||
        ((uintptr_t)p->le_c & 7))
        return SBCE_EINVAL;
    if (((uintptr_t)p->perm & 3) || ((uintptr_t)p->u_true & 3) || ((uintptr_t)p->u_hat & 3) ||
        ((uintptr_t)p->err & 3))
        return SBCE_EINVAL;
    if (p->workspace_bytes < siso_ws_bytes(d->batch, d->k, T)) return SBCE_EWORKSPACE;
    clear_stale_error();
    SisoArgs a{};
    a.lc = p->lc; a.la = p->la_u; a.perm = p->perm; a.utrue = p->u_true;
    a.lapp = p->lapp_u; a.uhat = p->u_hat; a.lec = p->le_c; a.err = p->err;
    a.ws = (double*)p->workspace;
    a.B = d->batch; a.ninfo = d->n_info; a.T = T; a.K = d->k; a.N = d->n;
    for (int j = 0; j < 3; ++j) a.g[j] = j < d->n ? d->gen[j] : 0;
    a.term = (d->flags & SBCE_SISO_TERMINATED) ? 1 : 0;
    a.maxlog = (d->flags & SBCE_DETECT_MAXLOG) ? 1 : 0;
    return hip_rc(launch_siso(a, (hipStream_t)hip_stream));
}

}  // extern "C"
