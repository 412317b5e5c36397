// Which of the 30 simulation walks a run launches: the one statement of the rule.  Plain C++ without a HIP header, so that sim_launch (sim_host.hpp),
// the six launchers and the stand-alone program of the tests (tests/cpp/sim_pick_table.cpp) share ONE copy of it.
#pragma once

namespace hs {

// what a run is asked for: the switches of the simulation object (hsddp_plant_set, hsddp_contact_set, hsddp_terrain_set, hsddp_substep_set,
// hsddp_grf_set) and of the run itself (mc: a disturbed run, hsddp_mc_run with something switched on; noise: one of its sigmas is above zero).  fric_on
// (hsddp_friction_set) is a trailing member with a default, so that a setting written before it existed means what it meant
struct SimSwitches { bool plant_on, uni_on, ter_on; int substeps; bool grf_on, mc, noise; bool fric_on = false; };

enum SimFamily { SIM_FAM_BASE, SIM_FAM_SUB, SIM_FAM_UNI, SIM_FAM_TER, SIM_FAM_PLANT, SIM_FAM_FRIC };      // wb_sim.hpp / hsddp_sub.hip / _uni / _ter / _plant / _fric: one launcher each
enum SimVariant { SIM_VAR_PLAIN, SIM_VAR_MC, SIM_VAR_MC0 };                               // no disturbance / with the generator / compiled without it
enum SimContact { SIM_BILATERAL, SIM_CONTACT_RULE, SIM_TERRAIN };                         // the contact model; the plant family has a twin for each
// records: the force records are the caller's (hsddp_grf_set has them on).  The base and sub-stepped families then launch their _grf twin; the other
// three always keep records and write them to the dummy block while this is false.
// unsupported: friction and the plant both act (hsddp_friction.h) - the pick is the plant's, and the run refuses with HSDDP_ENOTSUP instead of launching it.
struct SimPick { SimFamily family; SimVariant variant; bool records; SimContact contact; bool unsupported = false; };

// The rule.  The plant comes first; the terrain acts only while the contact rule is on; the contact rule, the terrain and the plant always carry the
// records and the sub-step loop (for one substep too); of the rest, more than one substep selects _sub and the records select _grf; a disturbed run
// takes _mc with noise and _mc0 without, and noise without mc means nothing.  Friction acts only while the contact rule is on, with the terrain on or off
// (three kernels serve both: the host binds a flat map for the latter, and contact says which it was); together with the plant it is flagged, not ignored.
inline SimPick sim_pick(const SimSwitches& s) {
    const bool ter = s.uni_on && s.ter_on;
    SimPick p;
    p.contact = ter ? SIM_TERRAIN : s.uni_on ? SIM_CONTACT_RULE : SIM_BILATERAL;
    const bool fric = s.uni_on && s.fric_on;
    p.unsupported = fric && s.plant_on;
    p.family = s.plant_on ? SIM_FAM_PLANT : fric ? SIM_FAM_FRIC : ter ? SIM_FAM_TER : s.uni_on ? SIM_FAM_UNI : s.substeps > 1 ? SIM_FAM_SUB : SIM_FAM_BASE;
    p.variant = !s.mc ? SIM_VAR_PLAIN : s.noise ? SIM_VAR_MC : SIM_VAR_MC0;
    p.records = s.grf_on;
    return p;
}

// the kernel a pick launches (columns: SimVariant)
inline const char* sim_kernel_name(const SimPick& p) {
    static const char* const names[10][3] = {
        {"k_sim_quad", "k_sim_quad_mc", "k_sim_quad_mc0"},
        {"k_sim_quad_grf", "k_sim_quad_mc_grf", "k_sim_quad_mc0_grf"},
        {"k_sim_quad_sub", "k_sim_quad_mc_sub", "k_sim_quad_mc0_sub"},
        {"k_sim_quad_grf_sub", "k_sim_quad_mc_grf_sub", "k_sim_quad_mc0_grf_sub"},
        {"k_sim_quad_uni", "k_sim_quad_mc_uni", "k_sim_quad_mc0_uni"},
        {"k_sim_quad_ter", "k_sim_quad_mc_ter", "k_sim_quad_mc0_ter"},
        {"k_sim_quad_plant", "k_sim_quad_mc_plant", "k_sim_quad_mc0_plant"},
        {"k_sim_quad_uni_plant", "k_sim_quad_mc_uni_plant", "k_sim_quad_mc0_uni_plant"},
        {"k_sim_quad_ter_plant", "k_sim_quad_mc_ter_plant", "k_sim_quad_mc0_ter_plant"},
        {"k_sim_quad_fric", "k_sim_quad_mc_fric", "k_sim_quad_mc0_fric"},
    };
    int row = 0;
    switch (p.family) {
        case SIM_FAM_BASE: row = p.records ? 1 : 0; break;
        case SIM_FAM_SUB: row = p.records ? 3 : 2; break;
        case SIM_FAM_UNI: row = 4; break;
        case SIM_FAM_TER: row = 5; break;
        case SIM_FAM_PLANT: row = 6 + (int)p.contact; break;
        case SIM_FAM_FRIC: row = 9; break;
    }
    return names[row][p.variant];
}

}  // namespace hs
