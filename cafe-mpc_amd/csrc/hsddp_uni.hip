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

// Records and the sub-step loop are always compiled in, so the parked column is that of the _grf_sub twins plus SIM_UNI_PARK doubles per lane (39 / 41:
// at most 20 992 B per wave).
WBS_KERNEL(k_sim_quad_uni, WbsUni, SIM_PARK + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK, WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un), gr, sb, un)
WBS_KERNEL(k_sim_quad_mc_uni, WbsMcUni<1>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un), mc, gr, sb, un)
WBS_KERNEL(k_sim_quad_mc0_uni, WbsMcUni<0>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un), mc, gr, sb, un)

void wbs_uni_launch(const WbsLaunch& L) {
    if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_uni, L.gr, L.sb, L.un);
    else wbs_launch(L, L.pick.variant == SIM_VAR_MC ? k_sim_quad_mc_uni : k_sim_quad_mc0_uni, L.mc, L.gr, L.sb, L.un);
}

}  // namespace hs
