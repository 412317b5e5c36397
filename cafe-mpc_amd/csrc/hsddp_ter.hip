// The simulation kernels with terrain height maps and early swing-foot touchdown of libhsddp_hip.so (include/hsddp_terrain.h; the walk is wbs_walk of
// wb_sim.hpp with TER 1 on top of UNI 1 in its policy) and their launcher.  The Makefile compiles this file on its own (-DHS_TER_SEPARATE for
// hsddp_hip.hip); hsddp_hip.hip includes it when it is built without that switch (a one-command build of the library).  A translation unit of its own
// for the reason given in hsddp_sub.hip and hsddp_uni.hip: the code objects of the other files have to keep every kernel where it is.
#ifdef HS_TER_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#include "wb_sim.hpp"
#endif

namespace hs {

#ifndef SIM_WPE
#define SIM_WPE 1
#endif
// The launch shape of the other walks: 64 lanes, sixteen quads per wave, one wave per SIMD.  The parked column is that of the _uni twins plus
// SIM_TER_PARK doubles per lane (45 / 47: at most 24 064 B per wave).
#define WBS_TER_KERNEL(NAME, POLICY, PARK, PARAMS, ...)                                                                                                                        \
    __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))                                                                               \
    NAME(const PhaseDev* ph_, ModelDev md, const int* map, int n_steps, int n_samples, int total, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU, \
         PARAMS const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te) {                                                                      \
        __shared__ double stash[((PARK) + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK) * 64];                                                                    \
        const int g = blockIdx.x * 16 + (threadIdx.x >> 2);                                                                                                                    \
        if (g >= total) return;                                                                                                                                                \
        wbs_walk<QS, POLICY>((PhaseC*)ph_, md, map, n_steps, g / n_samples, (size_t)g, x0, xfinal, rows, trajX, trajU, stash, POLICY{__VA_ARGS__});                            \
    }
#define WBS_P(...) __VA_ARGS__,
WBS_TER_KERNEL(k_sim_quad_ter, WbsTer, SIM_PARK, , gr, sb, un, te)
WBS_TER_KERNEL(k_sim_quad_mc_ter, WbsMcTer<1>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, gr, sb, un, te)
WBS_TER_KERNEL(k_sim_quad_mc0_ter, WbsMcTer<0>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, gr, sb, un, te)
#undef WBS_P
#undef WBS_TER_KERNEL

// The one launch of a run with the contact rule and the terrain on: mc null - the plain walk, else the disturbed one (noise: with the generator).  As
// wbs_uni_launch it leaves the runtime's error state to the caller.
void wbs_ter_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const ModelDev& md, const int* map, int n_steps, int n_samples, int total, const double* x0,
                    double* xfinal, double* rows, double* trajX, double* trajU, const WbsMcArgs* mc, bool noise, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un,
                    const WbsTerArgs* te) {
#define TER_LAUNCH(K, ...) hipLaunchKernelGGL(K, dim3(grid), dim3(64), 0, stream, ph, md, map, n_steps, n_samples, total, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (!mc) TER_LAUNCH(k_sim_quad_ter, gr, sb, un, te);
    else if (noise) TER_LAUNCH(k_sim_quad_mc_ter, mc, gr, sb, un, te);
    else TER_LAUNCH(k_sim_quad_mc0_ter, mc, gr, sb, un, te);
#undef TER_LAUNCH
}

}  // namespace hs
