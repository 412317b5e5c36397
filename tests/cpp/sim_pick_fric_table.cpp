// TEST-ONLY: a stand-alone program around the dispatch rule of the simulation walks WITH the friction switch (cafe-mpc_amd/csrc/sim_pick.hpp: which of the
// 30 kernels a run launches), for -fsanitize=address,undefined.  tests/test_friction_host.py compiles and runs it beside tests/cpp/sim_pick_table.cpp, which
// walks the 128 settings without the switch.  This one walks all 2^7 switch settings x substeps in {1, 2} = 256, compares the kernel the rule names with a
// name composed HERE from the suffix rules of the headers under include/, checks that exactly the 30 product walks are reachable, that friction without
// the contact rule is inert, that with the switch off the pick is the one of a setting written before the switch existed, and that friction together with
// the plant is flagged (and nothing else is), and prints "sim_pick_fric_table: clean" when everything answered as expected.
#include <cstdio>
#include <set>
#include <string>
#include "sim_pick.hpp"

using namespace hs;

static int failures = 0;
static void fail(const SimSwitches& s, const char* what, const std::string& got, const std::string& want) {
    std::printf("sim_pick_fric_table: plant %d uni %d ter %d substeps %d grf %d mc %d noise %d fric %d: %s: got %s, want %s\n", (int)s.plant_on, (int)s.uni_on, (int)s.ter_on,
                s.substeps, (int)s.grf_on, (int)s.mc, (int)s.noise, (int)s.fric_on, what, got.c_str(), want.c_str());
    failures++;
}

// the suffix rules of sim_pick_table.cpp, plus: _fric (hsddp_friction.h) in place of _uni / _ter while the contact rule and friction are both on - three
// kernels serve both ground models - unless the plant is on, which comes first
static std::string expected(const SimSwitches& s) {
    std::string n = "k_sim_quad";
    if (s.mc) n += s.noise ? "_mc" : "_mc0";
    if (s.plant_on || s.uni_on) {
        if (s.uni_on) n += (s.fric_on && !s.plant_on) ? "_fric" : s.ter_on ? "_ter" : "_uni";
        if (s.plant_on) n += "_plant";
    } else {
        if (s.grf_on) n += "_grf";
        if (s.substeps > 1) n += "_sub";
    }
    return n;
}

static bool same(const SimPick& a, const SimPick& b) { return a.family == b.family && a.variant == b.variant && a.records == b.records && a.contact == b.contact && a.unsupported == b.unsupported; }

int main() {
    const std::set<std::string> product = {
        "k_sim_quad", "k_sim_quad_mc", "k_sim_quad_mc0", "k_sim_quad_grf", "k_sim_quad_mc_grf", "k_sim_quad_mc0_grf",
        "k_sim_quad_sub", "k_sim_quad_mc_sub", "k_sim_quad_mc0_sub", "k_sim_quad_grf_sub", "k_sim_quad_mc_grf_sub", "k_sim_quad_mc0_grf_sub",
        "k_sim_quad_uni", "k_sim_quad_mc_uni", "k_sim_quad_mc0_uni", "k_sim_quad_ter", "k_sim_quad_mc_ter", "k_sim_quad_mc0_ter",
        "k_sim_quad_plant", "k_sim_quad_mc_plant", "k_sim_quad_mc0_plant", "k_sim_quad_uni_plant", "k_sim_quad_mc_uni_plant", "k_sim_quad_mc0_uni_plant",
        "k_sim_quad_ter_plant", "k_sim_quad_mc_ter_plant", "k_sim_quad_mc0_ter_plant", "k_sim_quad_fric", "k_sim_quad_mc_fric", "k_sim_quad_mc0_fric"};
    std::set<std::string> reached, reached_off;
    int settings = 0, flagged = 0;
    for (int bits = 0; bits < 128; bits++) for (int S = 1; S <= 2; S++, settings++) {
        SimSwitches s = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, S, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0};
        const SimPick old = sim_pick(s);      // the setting as it was written before the switch existed: the trailing member takes its default
        if (s.fric_on) fail(s, "the default of the switch", "on", "off");
        s.fric_on = (bits & 64) != 0;
        const SimPick p = sim_pick(s);
        const std::string got = sim_kernel_name(p), want = expected(s);
        if (got != want) fail(s, "the kernel", got, want);
        if (!product.count(got)) fail(s, "a kernel of the product build", got, "one of the 30");
        reached.insert(got);
        if (!s.fric_on) { reached_off.insert(got); if (!same(p, old)) fail(s, "the switch off", got, sim_kernel_name(old)); }
        if (p.records != s.grf_on) fail(s, "records", p.records ? "real" : "dummy", s.grf_on ? "real" : "dummy");
        if (!s.uni_on) {      // friction is dormant while the contact rule is off
            SimSwitches t = s; t.fric_on = !s.fric_on;
            if (!same(p, sim_pick(t))) fail(s, "friction without the contact rule", sim_kernel_name(sim_pick(t)), got);
        }
        const bool both = s.plant_on && s.uni_on && s.fric_on;      // friction acting together with the plant: flagged, never silently ignored
        if (p.unsupported != both) fail(s, "the plant combination", p.unsupported ? "flagged" : "not flagged", both ? "flagged" : "not flagged");
        if (p.unsupported && p.family != SIM_FAM_PLANT) fail(s, "the plant comes first", got, "a _plant kernel");
        if (p.family == SIM_FAM_FRIC && p.contact != (s.ter_on ? SIM_TERRAIN : SIM_CONTACT_RULE)) fail(s, "the ground model of a friction run", "other", s.ter_on ? "terrain" : "contact rule");
        flagged += p.unsupported ? 1 : 0;
    }
    if (settings != 256) { std::printf("sim_pick_fric_table: %d settings walked, want 256\n", settings); failures++; }
    if (flagged != 32) { std::printf("sim_pick_fric_table: %d settings flagged, want 32\n", flagged); failures++; }
    if (reached != product) {
        for (const std::string& k : product) if (!reached.count(k)) { std::printf("sim_pick_fric_table: %s is never launched\n", k.c_str()); failures++; }
    }
    if (reached.size() != 30) { std::printf("sim_pick_fric_table: %zu kernels reached, want 30\n", reached.size()); failures++; }
    if (reached_off.size() != 27) { std::printf("sim_pick_fric_table: %zu kernels reached with the switch off, want 27\n", reached_off.size()); failures++; }
    if (failures == 0) std::printf("sim_pick_fric_table: clean\n");
    return failures == 0 ? 0 : 1;
}
