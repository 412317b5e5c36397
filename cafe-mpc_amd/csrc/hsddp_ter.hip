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

// The parked column is that of the _uni twins plus SIM_TER_PARK doubles per lane (45 / 47: at most 24 064 B per wave).
WBS_KERNEL(k_sim_quad_ter, WbsTer, SIM_PARK + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK,
           WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te), gr, sb, un, te)
WBS_KERNEL(k_sim_quad_mc_ter, WbsMcTer<1>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK,
           WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te), mc, gr, sb, un, te)
WBS_KERNEL(k_sim_quad_mc0_ter, WbsMcTer<0>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK,
           WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te), mc, gr, sb, un, te)

void wbs_ter_launch(const WbsLaunch& L) {
    if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_ter, L.gr, L.sb, L.un, L.te);
    else wbs_launch(L, L.pick.variant == SIM_VAR_MC ? k_sim_quad_mc_ter : k_sim_quad_mc0_ter, L.mc, L.gr, L.sb, L.un, L.te);
}

}  // namespace hs
