// tests/cpp/episode_loop.cpp with per-robot policy latency (include/hsddp_latency.h) switched on through hsddp::Episode::set_latency: the plain walk, the
// log kept.  Prints one JSON object: the episode rows, the latency rows and the log X / U (tests compare them with the Python path bit for bit).
//   latency_loop <cafe_tree> <gait> <option.bin> <x0.bin: batch x 36 doubles> <batch> <start_window> <n_ticks> <delay of robot 0> ... <delay of robot batch-1>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "mhpc_builder.hpp"
#include "MultiPhaseDDP.hpp"

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const std::string root = argv[1], gait = argv[2], optfile = argv[3], x0file = argv[4];
    const int batch = std::atoi(argv[5]), start = std::atoi(argv[6]), n_ticks = std::atoi(argv[7]);
    if (argc != 8 + batch) return 2;
    std::vector<int> delay; for (int b = 0; b < batch; b++) delay.push_back(std::atoi(argv[8 + b]));
    hsddp::HSDDP_OPTION opt0 = hsddp::default_option();
    { std::ifstream f(optfile, std::ios::binary); if (!f.read(reinterpret_cast<char*>(&opt0), sizeof(opt0))) return 4; }
    hsddp::HSDDP_OPTION opt_rt = opt0; opt_rt.max_AL_iter = opt0.max_AL_iter_runtime; opt_rt.max_DDP_iter = opt0.max_DDP_iter_runtime;
    std::vector<double> x0((size_t)batch * 36);
    { std::ifstream f(x0file, std::ios::binary); if (!f.read(reinterpret_cast<char*>(x0.data()), x0.size() * sizeof(double))) return 4; }
    auto cfg = hsddp::load_mhpc_config(root + "/MHPC/settings/mhpc_config.info");
    auto costs = hsddp::load_cost_weights(root + "/" + cfg.costFile);
    auto cpar = hsddp::load_constraint_params(root + "/" + cfg.constraintParamFile);
    hsddp::QuadReference ref; if (!ref.load(root + "/Reference/Data/" + gait + "/quad_reference.csv", false)) return 3;
    hsddp::MhpcProblemData pd(ref, cfg, costs, cpar);
    for (int i = 0; i < start; i++) pd.update();
    std::vector<hsddp::PhaseBuffers> bufs; auto descs = pd.describe(bufs);
    std::vector<int> uids; for (auto& r : pd.wb) uids.push_back(r.uid); if (pd.srb_h > 0) uids.push_back(-1);
    const int nst = (int)std::round((double)cfg.dt_mpc / cfg.dt_wb);

    hsddp::MultiPhaseDDP<double> solver(batch, 0);
    solver.set_multiPhaseProblem(descs);
    if (solver.last_error()) { std::fprintf(stderr, "create failed: %d\n", solver.last_error()); return 5; }
    for (size_t i = 0; i < descs.size(); i++) solver.set_nominal((int)i, bufs[i].Xbar.data(), bufs[i].Ubar.data());
    hsddp::Episode ep(solver.handle(), batch, nst, n_ticks, true);
    if (ep.last_error() || !ep.set_latency(true, delay.data()) || !ep.reset(x0.data())) { std::fprintf(stderr, "episode failed: %d\n", ep.last_error()); return 5; }
    solver.solve(opt0);
    if (solver.last_error()) { std::fprintf(stderr, "initial solve failed: %d\n", solver.last_error()); return 6; }
    for (int tick = 0; tick < n_ticks; tick++) {
        if (!ep.advance(nullptr)) { std::fprintf(stderr, "advance failed at tick %d: %d\n", tick, ep.last_error()); return 7; }
        auto moves = pd.update();
        std::vector<hsddp::PhaseBuffers> nb; auto nd = pd.describe(nb);
        std::map<int, int> old_index; for (size_t i = 0; i < uids.size(); i++) old_index[uids[i]] = (int)i;
        std::vector<int> nu; for (auto& r : pd.wb) nu.push_back(r.uid); if (pd.srb_h > 0) nu.push_back(-1);
        std::vector<int> src(nu.size(), -1), shift(nu.size(), 0);
        for (size_t i = 0; i < nu.size(); i++) {
            if (nu[i] == -1) { src[i] = old_index[-1]; shift[i] = pd.srb_steps; }
            else if (old_index.count(nu[i])) { src[i] = old_index[nu[i]]; for (auto& mv : moves) if (mv.uid == nu[i]) shift[i] = mv.popped; }
        }
        solver.reconfigure(nd, src, shift);
        if (solver.last_error()) { std::fprintf(stderr, "reconfigure failed at tick %d: %d\n", tick, solver.last_error()); return 7; }
        solver.solve(opt_rt);
        if (solver.last_error()) { std::fprintf(stderr, "solve failed at tick %d: %d\n", tick, solver.last_error()); return 8; }
        descs = nd; bufs.swap(nb); uids = nu;
    }
    std::printf("{\"n_exec\":%d,\"rows\":[", nst);
    auto rows = ep.rows();
    for (int b = 0; b < batch; b++) {
        const hsddp_episode_row_t& r = rows[b];
        std::printf("%s{\"dev_q\":%.17g,\"dev_v\":%.17g,\"min_height\":%.17g,\"max_torque\":%.17g,\"track_cost\":%.17g,\"steps\":%d,\"bad_solves\":%d,\"end_reason\":%d,\"end_step\":%d}",
                    b ? "," : "", r.dev_q, r.dev_v, r.min_height, r.max_torque, r.track_cost, r.steps, r.bad_solves, r.end_reason, r.end_step);
    }
    std::printf("],\"latency\":[");
    auto lat = ep.latency();
    if (ep.last_error()) { std::fprintf(stderr, "latency rows failed: %d\n", ep.last_error()); return 9; }
    for (int b = 0; b < batch; b++) std::printf("%s[%d,%d]", b ? "," : "", lat[b].delay, lat[b].n_stale);
    auto log = ep.log();
    std::printf("],\"X\":[");
    for (size_t i = 0; i < log.X.size(); i++) std::printf("%s%.17g", i ? "," : "", log.X[i]);
    std::printf("],\"U\":[");
    for (size_t i = 0; i < log.U.size(); i++) std::printf("%s%.17g", i ? "," : "", log.U[i]);
    std::printf("]}\n");
    return 0;
}
