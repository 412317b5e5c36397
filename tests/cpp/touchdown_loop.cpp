// tests/cpp/episode_loop.cpp on a terrain, with terrain-aware planning (include/hsddp_touchdown.h): the contact rule and a height grid in the episode's
// simulation object, and per tick, between MultiPhaseDDP::reconfigure and the solve, Episode::plan_terrain() - the touchdown heights of the new window
// from the grid the episode simulates on.  Prints one JSON object: per tick the iterations and costs of every problem, the number of problems alive
// and the touchdown heights in use in phase <td_phase> after the solve, then the episode rows (tests compare them with the Python path,
// episode.run_mhpc(..., plan_terrain=True)).
//   touchdown_loop <cafe_tree> <gait> <option.bin> <x0.bin: batch x 36 doubles> <batch> <start_window> <n_ticks> <substeps> <H.bin: n_maps x ny x nx doubles>
//                  <nx> <ny> <n_maps> <x0> <y0> <cx> <cy> <map.bin: batch ints> <plan: 0 | 1>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "mhpc_builder.hpp"
#include "MultiPhaseDDP.hpp"

int main(int argc, char** argv) {
    if (argc < 19) return 2;
    const std::string root = argv[1], gait = argv[2], optfile = argv[3], x0file = argv[4];
    const int batch = std::atoi(argv[5]), start = std::atoi(argv[6]), n_ticks = std::atoi(argv[7]);
    const int substeps = std::atoi(argv[8]), plan = std::atoi(argv[18]);
    hsddp_terrain_t ter{}; ter.nx = std::atoi(argv[10]); ter.ny = std::atoi(argv[11]); ter.n_maps = std::atoi(argv[12]); ter.early = 1;
    ter.x0 = std::atof(argv[13]); ter.y0 = std::atof(argv[14]); ter.cx = std::atof(argv[15]); ter.cy = std::atof(argv[16]); ter.w_td = 0.0;
    std::vector<double> H((size_t)ter.n_maps * ter.ny * ter.nx); std::vector<int> map_of(batch);
    { std::ifstream f(argv[9], std::ios::binary); if (!f.read(reinterpret_cast<char*>(H.data()), H.size() * sizeof(double))) return 4; }
    { std::ifstream f(argv[17], std::ios::binary); if (!f.read(reinterpret_cast<char*>(map_of.data()), map_of.size() * sizeof(int))) return 4; }
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
    for (int i = 0; i < start; i++) pd.update();      // the builder advanced to the start window on the host
    std::vector<hsddp::PhaseBuffers> bufs; auto descs = pd.describe(bufs);
    std::vector<int> uids; for (auto& r : pd.wb) uids.push_back(r.uid); if (pd.srb_h > 0) uids.push_back(-1);
    const int nst = (int)std::round((double)cfg.dt_mpc / cfg.dt_wb);

    hsddp::MultiPhaseDDP<double> solver(batch, 0);
    solver.set_multiPhaseProblem(descs);
    if (solver.last_error()) { std::fprintf(stderr, "create failed: %d\n", solver.last_error()); return 5; }
    for (size_t i = 0; i < descs.size(); i++) solver.set_nominal((int)i, bufs[i].Xbar.data(), bufs[i].Ubar.data());
    hsddp::Episode ep(solver.handle(), batch, nst, n_ticks, false);
    if (ep.last_error() || !ep.set_substeps(substeps) || !ep.set_contact(true, 0.0, 0.0) || !ep.set_terrain(true, &ter, H.data(), map_of.data()) || !ep.reset(x0.data())) { std::fprintf(stderr, "episode failed: %d\n", ep.last_error()); return 5; }
    solver.solve(opt0);
    if (solver.last_error()) { std::fprintf(stderr, "initial solve failed: %d\n", solver.last_error()); return 6; }

    std::printf("{\"ticks\":%d,\"batch\":%d,\"n_exec\":%d,\"per_tick\":[", n_ticks, batch, nst);
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
        if (plan && !ep.plan_terrain()) { std::fprintf(stderr, "plan_terrain failed at tick %d: %d\n", tick, ep.last_error()); return 7; }
        solver.solve(opt_rt);
        if (solver.last_error()) { std::fprintf(stderr, "solve failed at tick %d: %d\n", tick, solver.last_error()); return 8; }
        int t = 0, alive = 0, imp = 0; ep.status(&t, &alive, &imp);
        std::printf("%s{\"alive\":%d,\"impacts\":%d,\"iters\":[", tick ? "," : "", alive, imp);
        for (int b = 0; b < batch; b++) { int a, l, r; float ms; solver.get_solver_info(a, l, r, ms, b); std::printf("%s%d", b ? "," : "", a); }
        std::printf("],\"cost\":[");
        for (int b = 0; b < batch; b++) std::printf("%s%.17g", b ? "," : "", solver.get_actual_cost(b));
        std::printf("],\"heights\":[");      // of the last phase of the window that has a touchdown constraint (none: empty)
        {
            std::vector<double> hts((size_t)batch * 4);
            int tdp = -1; for (size_t i = 0; i < nd.size(); i++) if (solver.touchdown((int)i, hts.data(), nullptr, 0, batch)) tdp = (int)i;
            if (tdp >= 0 && solver.touchdown(tdp, hts.data(), nullptr, 0, batch)) for (size_t i = 0; i < hts.size(); i++) std::printf("%s%.17g", i ? "," : "", hts[i]);
            std::printf("],\"td_phase\":%d", tdp);
        }
        std::printf("}");
        descs = nd; bufs.swap(nb); uids = nu;
    }
    std::printf("],\"rows\":[");
    std::vector<double> x; auto rows = ep.rows(&x);
    for (int b = 0; b < batch; b++) {
        const hsddp_episode_row_t& r = rows[b];
        std::printf("%s{\"dev_q\":%.17g,\"dev_v\":%.17g,\"min_height\":%.17g,\"max_torque\":%.17g,\"track_cost\":%.17g,\"n_sat\":%d,\"steps\":%d,\"bad_solves\":%d,\"end_reason\":%d,\"end_step\":%d}",
                    b ? "," : "", r.dev_q, r.dev_v, r.min_height, r.max_torque, r.track_cost, r.n_sat, r.steps, r.bad_solves, r.end_reason, r.end_step);
    }
    std::printf("],\"x_now\":[");
    for (size_t i = 0; i < x.size(); i++) std::printf("%s%.17g", i ? "," : "", x[i]);
    std::printf("]}\n");
    return 0;
}
