// The HKD-MPC receding-horizon loop of the reference on the reference-shaped C++ host path, with the command export at the end of every tick:
//   HKDMPCSolver::update (HKDMPC/HKDMPC.cpp:97-160): opt_problem.update(), xinit, solve with max_AL_iter = 2 / max_DDP_iter = 1,
//   update_foot_placement(), publish_mpc_cmd().
// Here: hsddp::HkdProblemData::update + describe (cafe-mpc_amd/host/mhpc_builder.hpp), hsddp::MultiPhaseDDP<double>::reconfigure /
// set_control_knot(0, 0) (HKDProblem.cpp:220) / set_initial_condition (the shifted plan's first state, as the Python loop does) / solve /
// export_hkd_command with the window's contact durations and the current footholds (the previous message's: there is no simulator here).
// Prints one JSON object: per tick the message words and their FNV-1a hash, the decoded footholds, the wall time split by call; the device
// allocations during the warm ticks (from tick 4 on).
//   hkd_mpc_loop <cafe_tree> <gait> <option.bin> <n_ticks>            (option.bin: the initial solve's hsddp_option_t)
//   hkd_mpc_loop <cafe_tree> <gait> builder <n_ticks>                 builder only, no device: per tick the phase table and contact durations
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include "mhpc_builder.hpp"
#include "MultiPhaseDDP.hpp"

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* c = (const unsigned char*)p; for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; } return h;
}

static void print_table(const hsddp::HkdProblemData& pd) {
    std::printf("[");
    for (size_t i = 0; i < pd.ph.size(); i++) {
        const auto& r = pd.ph[i];
        std::printf("%s{\"h\":%d,\"contact\":[%d,%d,%d,%d],\"dur\":[%.17g,%.17g,%.17g,%.17g]}", i ? "," : "", r.h, r.contact[0], r.contact[1], r.contact[2],
                    r.contact[3], r.dur[0], r.dur[1], r.dur[2], r.dur[3]);
    }
    std::printf("]");
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string root = argv[1], gait = argv[2], optfile = argv[3]; const int n_ticks = std::atoi(argv[4]);
    hsddp::QuadReference ref; if (!ref.load(root + "/Reference/Data/" + gait + "/quad_reference.csv", true)) return 3;
    hsddp::HkdProblemData pd(ref, hsddp::load_hkd_constraint_params(root + "/HKDMPC/settings/constraint_params.info"));
    if (optfile == "builder") {
        std::printf("{\"tables\":[");
        for (int tick = 0; tick <= n_ticks; tick++) { if (tick > 0) { pd.update(); std::printf(","); } print_table(pd); }
        std::printf("]}\n");
        return 0;
    }
    hsddp::HSDDP_OPTION opt0 = hsddp::default_option();
    { std::ifstream f(optfile, std::ios::binary); if (!f.read(reinterpret_cast<char*>(&opt0), sizeof(opt0))) return 4; }
    hsddp::HSDDP_OPTION opt_rt = opt0; opt_rt.max_AL_iter = 2; opt_rt.max_DDP_iter = 1;      // HKDMPC.cpp:102-103
    const int n_steps = 9; const double dt = 0.01, dt_mpc = 0.02;      // nsteps_between_mpc + 7 controls, knot step (HKDMPC.cpp:246-247, 281)
    auto durations = [&]() { std::vector<double> d; for (auto& r : pd.ph) d.insert(d.end(), r.dur.begin(), r.dur.end()); return d; };

    std::vector<hsddp::PhaseBuffers> bufs; auto descs = pd.describe(bufs);
    std::vector<int> uids; for (auto& r : pd.ph) uids.push_back(r.uid);
    hsddp::MultiPhaseDDP<double> solver(1, 0);
    solver.set_initial_condition(std::vector<double>(bufs[0].Xbar.begin(), bufs[0].Xbar.begin() + 24));
    solver.set_multiPhaseProblem(descs);
    if (solver.last_error()) { std::fprintf(stderr, "create failed: %d\n", solver.last_error()); return 5; }
    for (size_t i = 0; i < descs.size(); i++) solver.set_nominal((int)i, bufs[i].Xbar.data(), bufs[i].Ubar.data());
    solver.solve(opt0);
    if (solver.last_error()) { std::fprintf(stderr, "initial solve failed: %d\n", solver.last_error()); return 6; }
    // the initial message (HKDMPCSolver::initialize ends with the same two calls) from the reference's footholds at the start
    float pf[12]; { const hsddp::QuadSample& a = ref.at(0.f); for (int j = 0; j < 12; j++) pf[j] = (float)a.foot_pos[j]; }
    { auto d = durations(); auto w = solver.export_hkd_command(0, n_steps, 0.0, dt, d.data(), pf); if (solver.last_error()) return 7; std::memcpy(pf, &w[HSDDP_HKD_OFF_FOOT_PLACEMENT], 48); }

    struct Tick { double total, build, reconf, knot, state, setic, solve, exprt; std::vector<unsigned int> words; };
    std::vector<Tick> ticks;
    long long m0 = 0, m1 = 0;
    for (int tick = 1; tick <= n_ticks; tick++) {
        Tick T{}; auto t0 = clk::now(), ta = t0;
        auto moves = pd.update();
        std::vector<hsddp::PhaseBuffers> nb; auto nd = pd.describe(nb);
        std::map<int, int> old_index; for (size_t i = 0; i < uids.size(); i++) old_index[uids[i]] = (int)i;
        std::vector<int> nu; for (auto& r : pd.ph) nu.push_back(r.uid);
        std::vector<int> src(nu.size(), -1), shift(nu.size(), 0);
        for (size_t i = 0; i < nu.size(); i++)
            if (old_index.count(nu[i])) { src[i] = old_index[nu[i]]; for (auto& mv : moves) if (mv.uid == nu[i]) shift[i] = mv.popped; }
        const std::vector<double> dur = durations();
        T.build = ms_since(ta); ta = clk::now();
        solver.reconfigure(nd, src, shift);
        if (solver.last_error()) { std::fprintf(stderr, "reconfigure failed at tick %d: %d\n", tick, solver.last_error()); return 8; }
        T.reconf = ms_since(ta); ta = clk::now();
        solver.set_control_knot(0, 0, nullptr);
        T.knot = ms_since(ta); ta = clk::now();
        std::vector<double> x0 = solver.get_field(0, HSDDP_F_XBAR, 0, 1); x0.resize(24);      // the shifted plan's first state
        T.state = ms_since(ta); ta = clk::now();
        solver.set_initial_condition(x0);
        T.setic = ms_since(ta); ta = clk::now();
        solver.solve(opt_rt);
        T.solve = ms_since(ta); ta = clk::now();
        T.words = solver.export_hkd_command(0, n_steps, dt_mpc * tick, dt, dur.data(), pf);      // update_foot_placement + publish_mpc_cmd
        T.exprt = ms_since(ta);
        T.total = ms_since(t0);
        if (solver.last_error() || T.words[0] != (unsigned)n_steps) { std::fprintf(stderr, "tick %d failed: %d\n", tick, solver.last_error()); return 9; }
        std::memcpy(pf, &T.words[HSDDP_HKD_OFF_FOOT_PLACEMENT], 48);      // the commanded footholds stand in for the measured ones next tick
        ticks.push_back(std::move(T));
        descs = nd; bufs.swap(nb); uids = nu;
        if (tick == 4) m0 = hsddp_debug_malloc_count();
        m1 = hsddp_debug_malloc_count();
    }
    std::printf("{\"ticks\":%d,\"n_steps\":%d,\"device_allocations_in_warm_ticks\":%lld", n_ticks, n_steps, m1 - m0);
    const char* names[] = {"total", "descriptor_build", "reconfigure", "set_control_knot", "state_readback", "set_initial_condition", "solve", "export"};
    double Tick::*fields[] = {&Tick::total, &Tick::build, &Tick::reconf, &Tick::knot, &Tick::state, &Tick::setic, &Tick::solve, &Tick::exprt};
    for (int q = 0; q < 8; q++) {      // mean over the warm ticks (from tick 4 on), then every tick
        double mean = 0; int n = 0; for (size_t i = 3; i < ticks.size(); i++) { mean += ticks[i].*fields[q]; n++; }
        std::printf(",\"%s_ms_mean\":%.4f,\"%s_ms\":[", names[q], mean / std::max(n, 1), names[q]);
        for (size_t i = 0; i < ticks.size(); i++) std::printf("%s%.4f", i ? "," : "", ticks[i].*fields[q]);
        std::printf("]");
    }
    std::printf(",\"hash\":[");
    for (size_t i = 0; i < ticks.size(); i++) std::printf("%s\"%llu\"", i ? "," : "", (unsigned long long)fnv(ticks[i].words.data(), ticks[i].words.size() * 4));
    std::printf("],\"foot_placement\":[");
    for (size_t i = 0; i < ticks.size(); i++) {
        const float* f = reinterpret_cast<const float*>(&ticks[i].words[HSDDP_HKD_OFF_FOOT_PLACEMENT]);
        std::printf("%s[", i ? "," : ""); for (int j = 0; j < 12; j++) std::printf("%s%.9g", j ? "," : "", f[j]); std::printf("]");
    }
    std::printf("],\"rows\":[");
    for (size_t i = 0; i < ticks.size(); i++) {
        std::printf("%s[", i ? "," : ""); for (size_t j = 0; j < ticks[i].words.size(); j++) std::printf("%s%u", j ? "," : "", ticks[i].words[j]); std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}
