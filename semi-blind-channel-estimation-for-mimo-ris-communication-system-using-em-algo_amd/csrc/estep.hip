// E-step routing: which unit computes the per-symbol posterior moments of (pb, mode).
//   soft ZF / MMSE, expectation    estep_linear.hip (one kernel template over the kind; EP with
//   propagation                    a-priori L-values when EstepArgs::la is set)
//   PM / ZF / MMSE / Gauss         estep_pm.hip
//   exact soft / hard              the MFMA sweep (estep_sweep.hip) where one exists for the shape
//                                  (JA, JB >= 16), behind the preparation or the sphere pass
//                                  (estep_sphere.hip, estep_pair.hip) when the caller gave a
//                                  workspace; the VALU kernel (estep_valu.hip) everywhere else
#include "sbce_internal.h"

namespace sbce {

bool estep_supported(const Problem& pb, int mode) {
    if (estep_linear_mode(mode)) return estep_linear_supported(pb, mode);
    if (mode == SBCE_ESTEP_EP) return estep_ep_supported(pb);
    if (mode >= SBCE_ESTEP_PM && mode <= SBCE_ESTEP_GAUSS) return estep_pm_supported(pb, pb.pr, mode);
    return (mode == SBCE_ESTEP_SOFT || mode == SBCE_ESTEP_HARD) && estep_valu_supported(pb);
}

// The moment writers of launch_estep that fold EstepArgs::mchg: the tree pass's single-path store,
// the enumeration, the n_tx = 4 factorised-weight pass and the MFMA sweep (listed or not) -- every
// writer of a soft / hard E-step that takes the sweep branch below at n_tx >= 3.  Not the VALU
// kernel, the n_tx = 2 factorised passes (estep_pair.hip), the PM / ZF / MMSE / Gauss kernels or
// the soft ZF / MMSE and EP kernels (estep_linear.hip).
bool estep_momfold_supported(const Problem& pb, int mode) {
    if (mode != SBCE_ESTEP_SOFT && mode != SBCE_ESTEP_HARD) return false;
    return !g_debug.estep_valu && pb.NT >= 3 && estep_sweep_plan(pb).ok;
}

hipError_t launch_estep(const Problem& pb, const EstepArgs& a, int mode, hipStream_t s) {
    if (estep_linear_mode(mode) || mode == SBCE_ESTEP_EP) return launch_estep_linear(pb, a, mode, s);
    if (a.la) return hipErrorInvalidValue;   // the entry points accept a prior with EP only
    if (mode >= SBCE_ESTEP_PM && mode <= SBCE_ESTEP_GAUSS) return launch_estep_pm(pb, a, mode, pb.pr, s);
    const SweepPlan sp = estep_sweep_plan(pb);
    // SBCE_ESTEP_IMPL=valu: the VALU kernel at every shape (A/B runs)
    if (g_debug.estep_valu || !sp.ok) return launch_estep_valu(pb, a, mode, s);
    if (sp.blocks == 0) return hipSuccess;
    // without a workspace the sweep prepares each symbol itself; with one, the sphere pass runs
    // instead of the preparation pass where it exists (SBCE_ESTEP_SPHERE=0 disables: A/B)
    const bool sphere = a.prep && a.list && a.tree && pb.NR >= pb.NT && !g_debug.estep_nosphere;
    EstepArgs as = a;            // the passes' view: list only when the sphere pass runs
    if (!sphere) as.list = nullptr;
    if (a.prep) {
        const hipError_t e = sphere ? launch_estep_sphere(pb, as, sp, mode, s)
                                    : launch_estep_prep(pb, as, sp, mode, s);
        if (e != hipSuccess) return e;
    }
    // listed sweep: waves grab work until the list is exhausted, so a grid that fills the chip
    // (8 two-wave blocks per CU) is enough
    return launch_estep_sweep(pb, as, mode, sphere && sp.blocks > 2048 ? 2048 : sp.blocks, s);
}

}  // namespace sbce
