// TEST-ONLY: a stand-alone program around the dispatch rule of the simulation walks (cafe-mpc_amd/csrc/sim_pick.hpp: which of the 27 kernels a run launches),
// for -fsanitize=address,undefined.  tests/test_sim_host.py compiles and runs it.  It walks all 2^6 switch settings x substeps in {1, 2}, compares the
// kernel the rule names with a name composed HERE from the suffix rules of the headers under include/, checks that exactly the 27 product walks are
// reachable and that the documented inert combinations are inert, and prints "sim_pick_table: clean" when everything answered as expected.
#include <cstdio>
#include <set>
#include <string>
#include "sim_pick.hpp"

using namespace hs;

static int failures = 0;
static void fail(const SimSwitches& s, const char* what, const std::string& got, const std::string& want) {
    std::printf("sim_pick_table: plant %d uni %d ter %d substeps %d grf %d mc %d noise %d: %s: got %s, want %s\n", (int)s.plant_on, (int)s.uni_on, (int)s.ter_on, s.substeps,
                (int)s.grf_on, (int)s.mc, (int)s.noise, what, got.c_str(), want.c_str());
    failures++;
}

// k_sim_quad + _mc / _mc0 (hsddp_mc.h) + either _grf (hsddp_grf.h) + _sub (hsddp_substep.h), or _uni / _ter (hsddp_contact.h, hsddp_terrain.h: records and
// sub-step loop always, the terrain only on top of the contact rule) + _plant (hsddp_plant.h: on top of any of the three, records and loop always)
static std::string expected(const SimSwitches& s) {
    std::string n = "k_sim_quad";
    if (s.mc) n += s.noise ? "_mc" : "_mc0";
    if (s.plant_on || s.uni_on) {
        if (s.uni_on) n += s.ter_on ? "_ter" : "_uni";
        if (s.plant_on) n += "_plant";
    } else {
        if (s.grf_on) n += "_grf";
        if (s.substeps > 1) n += "_sub";
    }
    return n;
}

static bool same(const SimPick& a, const SimPick& b) { return a.family == b.family && a.variant == b.variant && a.records == b.records && a.contact == b.contact; }

int main() {
    // the kernels of the product build, as make resources, resources-ter and resources-plant list them
    const std::set<std::string> product = {
        "k_sim_quad", "k_sim_quad_mc", "k_sim_quad_mc0", "k_sim_quad_grf", "k_sim_quad_mc_grf", "k_sim_quad_mc0_grf",
        "k_sim_quad_sub", "k_sim_quad_mc_sub", "k_sim_quad_mc0_sub", "k_sim_quad_grf_sub", "k_sim_quad_mc_grf_sub", "k_sim_quad_mc0_grf_sub",
        "k_sim_quad_uni", "k_sim_quad_mc_uni", "k_sim_quad_mc0_uni", "k_sim_quad_ter", "k_sim_quad_mc_ter", "k_sim_quad_mc0_ter",
        "k_sim_quad_plant", "k_sim_quad_mc_plant", "k_sim_quad_mc0_plant", "k_sim_quad_uni_plant", "k_sim_quad_mc_uni_plant", "k_sim_quad_mc0_uni_plant",
        "k_sim_quad_ter_plant", "k_sim_quad_mc_ter_plant", "k_sim_quad_mc0_ter_plant"};
    std::set<std::string> reached;
    int settings = 0;
    for (int bits = 0; bits < 64; bits++) for (int S = 1; S <= 2; S++, settings++) {
        const SimSwitches s = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, S, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0};
        const SimPick p = sim_pick(s);
        const std::string got = sim_kernel_name(p), want = expected(s);
        if (got != want) fail(s, "the kernel", got, want);
        if (!product.count(got)) fail(s, "a kernel of the product build", got, "one of the 27");
        reached.insert(got);
        if (p.records != s.grf_on) fail(s, "records", p.records ? "real" : "dummy", s.grf_on ? "real" : "dummy");      // real records exactly while hsddp_grf_set has them on
        if (!s.uni_on) {      // the terrain is dormant while the contact rule is off
            SimSwitches t = s; t.ter_on = !s.ter_on;
            if (!same(p, sim_pick(t))) fail(s, "terrain without the contact rule", sim_kernel_name(sim_pick(t)), got);
        }
        if (!s.mc) {      // noise belongs to a disturbed run
            SimSwitches t = s; t.noise = !s.noise;
            if (!same(p, sim_pick(t))) fail(s, "noise without mc", sim_kernel_name(sim_pick(t)), got);
        }
    }
    if (settings != 128) { std::printf("sim_pick_table: %d settings walked, want 128\n", settings); failures++; }
    if (reached != product) {
        for (const std::string& k : product) if (!reached.count(k)) { std::printf("sim_pick_table: %s is never launched\n", k.c_str()); failures++; }
    }
    if (reached.size() != 27) { std::printf("sim_pick_table: %zu kernels reached, want 27\n", reached.size()); failures++; }
    if (failures == 0) std::printf("sim_pick_table: clean\n");
    return failures == 0 ? 0 : 1;
}
