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

// Three more doubles per lane in the parked column (27 / 29 doubles without records, 32 / 34 with them: at most 17 408 B per wave); sb points at the
// trip count in device memory.
WBS_KERNEL(k_sim_quad_sub, WbsSub, SIM_PARK + SIM_SUB_PARK, WBS_P(const WbsSubArgs* sb), sb)
WBS_KERNEL(k_sim_quad_mc_sub, WbsMcSub<1>, SIM_PARK_MC + SIM_SUB_PARK, WBS_P(const WbsMcArgs* mc, const WbsSubArgs* sb), mc, sb)
WBS_KERNEL(k_sim_quad_mc0_sub, WbsMcSub<0>, SIM_PARK_MC + SIM_SUB_PARK, WBS_P(const WbsMcArgs* mc, const WbsSubArgs* sb), mc, sb)
WBS_KERNEL(k_sim_quad_grf_sub, WbsGrfSub, SIM_PARK + SIM_GRF_PARK + SIM_SUB_PARK, WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb), gr, sb)
WBS_KERNEL(k_sim_quad_mc_grf_sub, WbsMcGrfSub<1>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb), mc, gr, sb)
WBS_KERNEL(k_sim_quad_mc0_grf_sub, WbsMcGrfSub<0>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb), mc, gr, sb)

void wbs_sub_launch(const WbsLaunch& L) {
    const bool noise = L.pick.variant == SIM_VAR_MC;
    if (!L.pick.records) {
        if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_sub, L.sb);
        else wbs_launch(L, noise ? k_sim_quad_mc_sub : k_sim_quad_mc0_sub, L.mc, L.sb);
    } else {
        if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_grf_sub, L.gr, L.sb);
        else wbs_launch(L, noise ? k_sim_quad_mc_grf_sub : k_sim_quad_mc0_grf_sub, L.mc, L.gr, L.sb);
    }
}

}  // namespace hs
