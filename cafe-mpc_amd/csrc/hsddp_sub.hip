// The sub-stepped simulation kernels of libhsddp_hip.so (include/hsddp_substep.h; the walk is wbs_walk of wb_sim.hpp with SUB 1 in its policy) and
// their launcher.  The Makefile compiles this file on its own (-DHS_SUB_SEPARATE for hsddp_hip.hip); hsddp_hip.hip includes it when it is built
// without that switch (a one-command build of the library).
// Why a translation unit of its own: the six kernels without the switch have to stay what they are - code AND placement.  With the six below in
// hsddp_hip.hip's code object every existing kernel kept its instructions, byte for byte, but moved by 0x2800 within the object, and the noisy
// walk k_sim_quad_mc - 75 KB of code, more than the 64 KB instruction cache - measured 18.81 - 18.84 ms against the parent build's 18.60 in
// alternated runs (config 3 x 16 samples x 200 steps; the two kernels that fit the cache did not move: 9.82 / 9.82 and 10.30 / 10.31 ms).  In a
// code object of their own the new kernels leave the old object exactly as it was.
#ifdef HS_SUB_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#include "wb_sim.hpp"
#endif

namespace hs {

#ifndef SIM_WPE
#define SIM_WPE 1
#endif
// The same launch shape as the kernels of wb_sim.hpp: 64 lanes, sixteen quads per wave, one wave per SIMD; three more doubles per lane in the parked
// column (27 / 29 doubles without records, 32 / 34 with them: at most 17 408 B per wave); sb points at the trip count in device memory.
#define WBS_SUB_KERNEL(NAME, POLICY, PARK, PARAMS, ...)                                                                                                                        \
    __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))                                                                               \
    NAME(const PhaseDev* ph_, ModelDev md, const int* map, int n_steps, int n_samples, int total, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU, \
         PARAMS const WbsSubArgs* sb) {                                                                                                                                        \
        __shared__ double stash[((PARK) + SIM_SUB_PARK) * 64];                                                                                                                 \
        const int g = blockIdx.x * 16 + (threadIdx.x >> 2);                                                                                                                    \
        if (g >= total) return;                                                                                                                                                \
        wbs_walk<QS, POLICY>((PhaseC*)ph_, md, map, n_steps, g / n_samples, (size_t)g, x0, xfinal, rows, trajX, trajU, stash, POLICY{__VA_ARGS__});                            \
    }
#define WBS_P(...) __VA_ARGS__,
WBS_SUB_KERNEL(k_sim_quad_sub, WbsSub, SIM_PARK, , sb)
WBS_SUB_KERNEL(k_sim_quad_mc_sub, WbsMcSub<1>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, sb)
WBS_SUB_KERNEL(k_sim_quad_mc0_sub, WbsMcSub<0>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc, sb)
WBS_SUB_KERNEL(k_sim_quad_grf_sub, WbsGrfSub, SIM_PARK + SIM_GRF_PARK, WBS_P(const WbsGrfArgs* gr), gr, sb)
WBS_SUB_KERNEL(k_sim_quad_mc_grf_sub, WbsMcGrfSub<1>, SIM_PARK_MC + SIM_GRF_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr), mc, gr, sb)
WBS_SUB_KERNEL(k_sim_quad_mc0_grf_sub, WbsMcGrfSub<0>, SIM_PARK_MC + SIM_GRF_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr), mc, gr, sb)
#undef WBS_P
#undef WBS_SUB_KERNEL

// The one launch of a sub-stepped run: mc null - the plain walk, else the disturbed one (noise: with the generator); gr null - without records.
// It does not look at the runtime's error state: a launch that fails is reported by the caller's hipGetLastError, as for the kernels of wb_sim.hpp
// (reading the error here would reset it and hide the failure from that check).
void wbs_sub_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const ModelDev& md, const int* map, int n_steps, int n_samples, int total, const double* x0,
                    double* xfinal, double* rows, double* trajX, double* trajU, const WbsMcArgs* mc, bool noise, const WbsGrfArgs* gr, const WbsSubArgs* sb) {
#define SUB_LAUNCH(K, ...) hipLaunchKernelGGL(K, dim3(grid), dim3(64), 0, stream, ph, md, map, n_steps, n_samples, total, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (!gr) {
        if (!mc) SUB_LAUNCH(k_sim_quad_sub, sb);
        else if (noise) SUB_LAUNCH(k_sim_quad_mc_sub, mc, sb);
        else SUB_LAUNCH(k_sim_quad_mc0_sub, mc, sb);
    } else {
        if (!mc) SUB_LAUNCH(k_sim_quad_grf_sub, gr, sb);
        else if (noise) SUB_LAUNCH(k_sim_quad_mc_grf_sub, mc, gr, sb);
        else SUB_LAUNCH(k_sim_quad_mc0_grf_sub, mc, gr, sb);
    }
#undef SUB_LAUNCH
}

}  // namespace hs
