// The simulation kernels with unilateral ground contact of libhsddp_hip.so (include/hsddp_contact.h; the walk is wbs_walk of wb_sim.hpp with UNI 1 in
// its policy) and their launcher.  The Makefile compiles this file on its own (-DHS_UNI_SEPARATE for hsddp_hip.hip); hsddp_hip.hip includes it when it
// is built without that switch (a one-command build of the library).  A translation unit of its own for the reason given in hsddp_sub.hip: the code
// object of hsddp_hip.hip has to keep every kernel where it is.
#ifdef HS_UNI_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#include "wb_sim.hpp"
#endif

namespace hs {

#ifndef SIM_WPE
#define SIM_WPE 1
#endif
// The launch shape of the other walks: 64 lanes, sixteen quads per wave, one wave per SIMD.  Records and the sub-step loop are always compiled in, so
// the parked column is that of the _grf_sub twins plus SIM_UNI_PARK doubles per lane (39 / 41: at most 20 992 B per wave).
#define WBS_UNI_KERNEL(NAME, POLICY, PARK, PARAMS, ...)                                                                                                                        \
    __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))                                                                               \
    NAME(const PhaseDev* ph_, ModelDev md, const int* map, int n_steps, int n_samples, int total, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU, \
         PARAMS const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un) {                                                                                            \
        __shared__ double stash[((PARK) + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK) * 64];                                                                                   \
        const int g = blockIdx.x * 16 + (threadIdx.x >> 2);                                                                                                                    \
        if (g >= total) return;                                                                                                                                                \
        wbs_walk<QS, POLICY>((PhaseC*)ph_, md, map, n_steps, g / n_samples, (size_t)g, x0, xfinal, rows, trajX, trajU, stash, POLICY{__VA_ARGS__});                            \
    }
#define WBS_P(...) __VA_ARGS__,
WBS_UNI_KERNEL(k_sim_quad_uni, WbsUni, SIM_PARK, , gr, sb, un)
WBS_UNI_KERNEL(k_sim_quad_mc_uni, WbsMcUni<1>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, gr, sb, un)
WBS_UNI_KERNEL(k_sim_quad_mc0_uni, WbsMcUni<0>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, gr, sb, un)
#undef WBS_P
#undef WBS_UNI_KERNEL

// The one launch of a run with the rule on: mc null - the plain walk, else the disturbed one (noise: with the generator).  As wbs_sub_launch it leaves
// the runtime's error state to the caller.
void wbs_uni_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const ModelDev& md, const int* map, int n_steps, int n_samples, int total, const double* x0,
                    double* xfinal, double* rows, double* trajX, double* trajU, const WbsMcArgs* mc, bool noise, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un) {
#define UNI_LAUNCH(K, ...) hipLaunchKernelGGL(K, dim3(grid), dim3(64), 0, stream, ph, md, map, n_steps, n_samples, total, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (!mc) UNI_LAUNCH(k_sim_quad_uni, gr, sb, un);
    else if (noise) UNI_LAUNCH(k_sim_quad_mc_uni, mc, gr, sb, un);
    else UNI_LAUNCH(k_sim_quad_mc0_uni, mc, gr, sb, un);
#undef UNI_LAUNCH
}

}  // namespace hs
