// The simulation kernels with a per-sample plant of libhsddp_hip.so (include/hsddp_plant.h; the walk is wbs_walk of wb_sim.hpp with PLANT 1 in its policy,
// on top of each of the three families) and their launchers.  The Makefile compiles this file on its own (-DHS_PLANT_SEPARATE for hsddp_hip.hip);
// hsddp_hip.hip includes it when it is built without that switch (a one-command build of the library).  A translation unit of its own for the reason
// given in hsddp_sub.hip, hsddp_uni.hip and hsddp_ter.hip: the code objects of the other files have to keep every kernel where it is.
#ifdef HS_PLANT_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#include "wb_sim.hpp"
#endif

namespace hs {

// Nothing of the row is parked, so the parked column is that of the twin WITH records and sub-step loop: 32 / 34 doubles per lane for the bilateral
// walks, 39 / 41 with the contact rule, 45 / 47 with the terrain (at most 24 064 B per wave).
#define PARK_B (SIM_GRF_PARK + SIM_SUB_PARK)
#define PARK_U (PARK_B + SIM_UNI_PARK)
#define PARK_T (PARK_U + SIM_TER_PARK)
WBS_KERNEL(k_sim_quad_plant, WbsPlant, SIM_PARK + PARK_B, WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsPlantArgs* pl), gr, sb, pl)
WBS_KERNEL(k_sim_quad_mc_plant, WbsMcPlant<1>, SIM_PARK_MC + PARK_B, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsPlantArgs* pl), mc, gr, sb, pl)
WBS_KERNEL(k_sim_quad_mc0_plant, WbsMcPlant<0>, SIM_PARK_MC + PARK_B, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsPlantArgs* pl), mc, gr, sb, pl)
WBS_KERNEL(k_sim_quad_uni_plant, WbsUniPlant, SIM_PARK + PARK_U, WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsPlantArgs* pl), gr, sb, un, pl)
WBS_KERNEL(k_sim_quad_mc_uni_plant, WbsMcUniPlant<1>, SIM_PARK_MC + PARK_U, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsPlantArgs* pl), mc, gr, sb, un, pl)
WBS_KERNEL(k_sim_quad_mc0_uni_plant, WbsMcUniPlant<0>, SIM_PARK_MC + PARK_U, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsPlantArgs* pl), mc, gr, sb, un, pl)
WBS_KERNEL(k_sim_quad_ter_plant, WbsTerPlant, SIM_PARK + PARK_T, WBS_P(const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsPlantArgs* pl), gr, sb, un, te, pl)
WBS_KERNEL(k_sim_quad_mc_ter_plant, WbsMcTerPlant<1>, SIM_PARK_MC + PARK_T, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsPlantArgs* pl), mc, gr, sb, un, te, pl)
WBS_KERNEL(k_sim_quad_mc0_ter_plant, WbsMcTerPlant<0>, SIM_PARK_MC + PARK_T, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr, const WbsSubArgs* sb, const WbsUniArgs* un, const WbsTerArgs* te, const WbsPlantArgs* pl), mc, gr, sb, un, te, pl)
#undef PARK_T
#undef PARK_U
#undef PARK_B

// The pending reset map of an episode on each robot's own plant (k_episode_impact of episode.hpp is its twin): grid = ceil(B / 16) waves of sixteen quads.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))
k_episode_impact_plant(const PhaseDev* ph_, ModelDev md, int pi, int total, const int* frozen, int stride, double* state, double* x0, const WbsPlantArgs* pl) {
    const int g = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (g >= total) return;      // (a quad leaves or stays as a whole)
    wbs_plant_impact<QS>((PhaseC*)ph_, md, pi, (size_t)g, frozen, stride, state, x0, pl);
}

// the _plant twin of the family the pick's contact model names
void wbs_plant_launch(const WbsLaunch& L) {
    const bool plain = L.pick.variant == SIM_VAR_PLAIN, noise = L.pick.variant == SIM_VAR_MC;
    if (L.pick.contact == SIM_BILATERAL) {
        if (plain) wbs_launch(L, k_sim_quad_plant, L.gr, L.sb, L.pl);
        else wbs_launch(L, noise ? k_sim_quad_mc_plant : k_sim_quad_mc0_plant, L.mc, L.gr, L.sb, L.pl);
    } else if (L.pick.contact == SIM_CONTACT_RULE) {
        if (plain) wbs_launch(L, k_sim_quad_uni_plant, L.gr, L.sb, L.un, L.pl);
        else wbs_launch(L, noise ? k_sim_quad_mc_uni_plant : k_sim_quad_mc0_uni_plant, L.mc, L.gr, L.sb, L.un, L.pl);
    } else {
        if (plain) wbs_launch(L, k_sim_quad_ter_plant, L.gr, L.sb, L.un, L.te, L.pl);
        else wbs_launch(L, noise ? k_sim_quad_mc_ter_plant : k_sim_quad_mc0_ter_plant, L.mc, L.gr, L.sb, L.un, L.te, L.pl);
    }
}

void wbs_plant_impact_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const ModelDev& md, int pi, int total, const int* frozen, int stride, double* state, double* x0,
                             const WbsPlantArgs* pl) {
    hipLaunchKernelGGL(k_episode_impact_plant, dim3(grid), dim3(64), 0, stream, ph, md, pi, total, frozen, stride, state, x0, pl);
}

}  // namespace hs
