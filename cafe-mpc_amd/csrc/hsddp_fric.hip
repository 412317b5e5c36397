// The simulation kernels with Coulomb friction of libhsddp_hip.so (include/hsddp_friction.h; the walk is wbs_walk of wb_sim.hpp with FRIC 1 on top of
// UNI 1 and TER 1 in its policy) and their launcher.  The Makefile compiles this file on its own (-DHS_FRIC_SEPARATE for hsddp_hip.hip); hsddp_hip.hip
// includes it when it is built without that switch (a one-command build of the library).  A translation unit of its own for the reason given in
// hsddp_sub.hip, hsddp_uni.hip and hsddp_ter.hip: the code objects of the other files have to keep every kernel where it is.  Three kernels serve both
// ground models: with the terrain off the host binds a one-cell flat map with early = 0, on which the _ter walk is the contact rule alone.
// The Makefile links this file's object into a library of its own, libhsddp_fric.so, which libhsddp_hip.so needs and finds beside itself: nothing here
// calls into the rest of the library (the launch record and the walk are headers), and libhsddp_hip.so's fat binary stays what it was.
#ifdef HS_FRIC_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#include "wb_sim.hpp"
#endif

namespace hs {

// The parked column is that of the _ter twins plus SIM_FRIC_PARK doubles per lane (56 / 58: at most 29 696 B per wave).
WBS_KERNEL(k_sim_quad_fric, WbsFric, SIM_PARK + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK + SIM_FRIC_PARK,
           WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsFricArgs* fc), gr, sb, un, te, fc)
WBS_KERNEL(k_sim_quad_mc_fric, WbsMcFric<1>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK + SIM_FRIC_PARK,
           WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsFricArgs* fc), mc, gr, sb, un, te, fc)
WBS_KERNEL(k_sim_quad_mc0_fric, WbsMcFric<0>, SIM_PARK_MC + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK + SIM_FRIC_PARK,
           WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsFricArgs* fc), mc, gr, sb, un, te, fc)

void wbs_fric_launch(const WbsLaunch& L) {
    if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_fric, L.gr, L.sb, L.un, L.te, L.fc);
    else wbs_launch(L, L.pick.variant == SIM_VAR_MC ? k_sim_quad_mc_fric : k_sim_quad_mc0_fric, L.mc, L.gr, L.sb, L.un, L.te, L.fc);
}

}  // namespace hs
