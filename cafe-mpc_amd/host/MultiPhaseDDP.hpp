// C++ host-side mirror of the reference solver surface, over the C-ABI of include/hsddp.h.
//
// Same method names / argument meaning as MultiPhaseDDP<T> (HSDDPSolver/header/MultiPhaseDDP.h:22-93) so that
// reference-shaped host code (problem builders, MPC drivers) can switch solvers by changing one type:
//     hsddp::MultiPhaseDDP<double> solver;                     // reference: MultiPhaseDDP<double> solver;
//     solver.set_initial_condition(x0);                        //   same
//     solver.set_multiPhaseProblem(phases);                    //   deque<shared_ptr<SinglePhaseBase>> -> descriptors
//     solver.solve(ddp_setting, max_cputime_ms);               //   same
//     solver.get_solver_info(n_iters, n_ls, n_reg, ms);        //   same
// The reference passes closures (SinglePhase.h:65-96); a GPU cannot call them, so phases are the POD descriptors
// `hsddp_phase_desc_t` (what MHPCProblem::create_problem_one_phase binds, MHPCProblem.cpp:403-601).  Error
// behaviour follows the reference (void returns, failures reported through status/prints); `last_error()` exposes
// the C-ABI return code that the reference has no equivalent of.  Header-only, no Eigen needed (plain vectors).
#pragma once
#include <vector>
#include <stdexcept>
#include <cstring>
#include "hsddp.h"
#include "hsddp_hkd.h"
#include "hsddp_refs.h"
#include "hsddp_sim.h"
#include "hsddp_mc.h"
#include "hsddp_grf.h"
#include "hsddp_substep.h"
#include "hsddp_contact.h"
#include "hsddp_terrain.h"
#include "hsddp_friction.h"
#include "hsddp_plant.h"
#include "hsddp_episode.h"
#include "hsddp_latency.h"
#include "hsddp_touchdown.h"
#include "hsddp_weights.h"
#include "hsddp_limits.h"

namespace hsddp {

using HSDDP_OPTION = hsddp_option_t;

inline HSDDP_OPTION default_option() {   // HSDDP_CompoundTypes.h:15-36 defaults
    HSDDP_OPTION o{};
    o.alpha = 0.1; o.gamma = 0.1; o.update_penalty = 8; o.update_relax = 0.1; o.update_regularization = 2; o.update_ReB = 7;
    o.max_DDP_iter = 3; o.max_AL_iter = 2; o.max_DDP_iter_runtime = 1; o.max_AL_iter_runtime = 2;
    o.cost_thresh = 1e-3; o.tconstr_thresh = 1e-3; o.pconstr_thresh = 1e-3; o.dynamics_feas_thresh = 1e-3;
    o.merit_rho = 1e4; o.merit_scale = 0.2; o.merit_offset = 10; o.AL_active = 1; o.ReB_active = 1; o.smooth_active = 0; o.MS = 1; o.nsteps_per_node = 1;
    return o;
}

// Closed-loop rollouts of a solved policy (include/hsddp_sim.h): one device object on a solver's handle, kept across MPC ticks (run() makes no
// device allocation).  Stale after MultiPhaseDDP::reconfigure (run() then fails with HSDDP_EINVAL: make a new one); destroy it before the solver.
struct SimResult {
    std::vector<hsddp_sim_row_t> rows;      // batch x n_samples
    std::vector<double> x_final;            // batch x n_samples x 36
    std::vector<double> X, U;               // keep_traj: batch x n_samples x (n_steps + 1) x 36, batch x n_samples x n_steps x 12
    std::vector<hsddp_mc_extra_t> extra;    // batch x n_samples after a disturbed run (include/hsddp_mc.h), else empty
    std::vector<hsddp_grf_row_t> grf;       // batch x n_samples after a run with the contact-force records on (include/hsddp_grf.h), else empty
    std::vector<double> Y;                  // ... and with keep_traj the contact forces, batch x n_samples x n_steps x 12
};
inline hsddp_mc_dist_t default_disturbance() { return hsddp_mc_dist_t{}; }      // every switch off
class Simulation {
public:
    Simulation(hsddp_handle_t* h, int batch, int n_samples, int n_steps, bool keep_traj = false) : batch_(batch), R_(n_samples), n_(n_steps), keep_(keep_traj) {
        rc_ = hsddp_sim_create(h, n_samples, n_steps, keep_traj ? 1 : 0, &s_);
        if (rc_ != HSDDP_OK) s_ = nullptr;
    }
    ~Simulation() { if (s_) hsddp_sim_destroy(s_); }
    Simulation(const Simulation&) = delete;
    Simulation& operator=(const Simulation&) = delete;
    // x0: batch x n_samples x 36 (host memory, or device memory with src_device = 1)
    bool run(const double* x0, int src_device = 0) { rc_ = s_ ? hsddp_sim_run(s_, x0, src_device) : HSDDP_EINVAL; if (rc_ == HSDDP_OK) { mc_ = false; grf_run_ = grf_; } return rc_ == HSDDP_OK; }
    // disturbed run: actuator / estimate noise, torque limit, fall height, and a push kick (batch x n_samples x 36, or null) at dist.kick_step
    bool run(const double* x0, const hsddp_mc_dist_t& dist, const double* kick, int src_device = 0, int kick_device = 0) {
        rc_ = s_ ? hsddp_mc_run(s_, x0, src_device, &dist, kick, kick_device) : HSDDP_EINVAL;
        if (rc_ == HSDDP_OK) { mc_ = true; grf_run_ = grf_; }
        return rc_ == HSDDP_OK;
    }
    // contact-force records for every later run: mu > 0 on with these thresholds, mu == 0 off (include/hsddp_grf.h)
    bool set_grf(double mu, double fz_min = 0.0) { rc_ = s_ ? hsddp_grf_set(s_, mu, fz_min) : HSDDP_EINVAL; if (rc_ == HSDDP_OK) grf_ = mu > 0.0; return rc_ == HSDDP_OK; }
    // sub-stepped integration for every later run: S Euler steps of dt / S per control knot under the knot's torque, 1 <= S <= 64 (include/hsddp_substep.h)
    bool set_substeps(int substeps) { rc_ = s_ ? hsddp_substep_set(s_, substeps) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    int substeps() { int v = 1; rc_ = s_ ? hsddp_substep_get(s_, &v) : HSDDP_EINVAL; return v; }
    // unilateral ground contact for every later run (include/hsddp_contact.h): on, the release threshold of the normal force, the height of the ground
    bool set_contact(bool on, double fz_rel = 0.0, double z_ground = 0.0) { rc_ = s_ ? hsddp_contact_set(s_, on ? 1 : 0, fz_rel, z_ground) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // rows of the last run, which has to be one with the rule on: batch x n_samples
    bool contact(hsddp_contact_row_t* rows) { rc_ = s_ ? hsddp_contact_get(s_, 0, batch_, rows) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // terrain height maps and early swing-foot touchdown for every later run with the contact rule on (include/hsddp_terrain.h): H [n_maps][ny][nx] and
    // map_of [batch][n_samples] (or null: map 0) are host arrays, copied by the call; on = false ignores the rest
    bool set_terrain(bool on, const hsddp_terrain_t* t = nullptr, const double* H = nullptr, const int* map_of = nullptr) { rc_ = s_ ? hsddp_terrain_set(s_, on ? 1 : 0, t, H, map_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // Coulomb friction for every later run with the contact rule on (include/hsddp_friction.h): mu [n_mu][2] rows (mu_s, mu_k), mu_of [batch][n_samples]
    // or null; rows of the last run, which has to be one with the contact rule and friction on: batch x n_samples
    bool set_friction(bool on, const hsddp_friction_t* f = nullptr, const double* mu = nullptr, const int* mu_of = nullptr) { rc_ = s_ ? hsddp_friction_set(s_, on ? 1 : 0, f, mu, mu_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    bool friction(hsddp_friction_row_t* rows) { rc_ = s_ ? hsddp_friction_get(s_, 0, batch_, rows) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // rows of the last run, which has to be one with the contact rule and the terrain on: batch x n_samples
    bool terrain(hsddp_terrain_row_t* rows) { rc_ = s_ ? hsddp_terrain_get(s_, 0, batch_, rows) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // a plant row per sample for every later run (include/hsddp_plant.h): P [n_plants][HSDDP_PLANT_ROW] and plant_of [batch][n_samples] (or null: row 0)
    // are host arrays, copied by the call; on = false ignores the rest
    bool set_plant(bool on, int n_plants = 0, const double* P = nullptr, const int* plant_of = nullptr) { rc_ = s_ ? hsddp_plant_set(s_, on ? 1 : 0, n_plants, P, plant_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // the table later runs use: n_plants x HSDDP_PLANT_ROW doubles (empty on a fresh object); on (optional): whether the plant is switched on
    std::vector<double> plant(bool* on = nullptr) {
        int o = 0, n = 0; std::vector<double> P;
        rc_ = s_ ? hsddp_plant_get_params(s_, &o, &n) : HSDDP_EINVAL;
        if (rc_ == HSDDP_OK && n > 0) { P.resize((size_t)n * HSDDP_PLANT_ROW); rc_ = hsddp_plant_get_table(s_, 0, n, P.data()); }
        if (on) *on = o != 0;
        return P;
    }
    // the records of the last run alone (result() holds them too): rows batch x n_samples, Y batch x n_samples x n_steps x 12 or null
    bool grf(hsddp_grf_row_t* rows, double* Y = nullptr) { rc_ = s_ ? hsddp_grf_get(s_, 0, batch_, rows, Y) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    SimResult result() {
        SimResult r;
        if (!s_) return r;
        const size_t cnt = (size_t)batch_ * R_;
        r.rows.resize(cnt); r.x_final.resize(cnt * 36);
        rc_ = hsddp_sim_get_rows(s_, 0, batch_, r.rows.data(), r.x_final.data());
        if (rc_ == HSDDP_OK && keep_) {
            r.X.resize(cnt * (size_t)(n_ + 1) * 36); r.U.resize(cnt * (size_t)n_ * 12);
            rc_ = hsddp_sim_get_traj(s_, 0, batch_, r.X.data(), r.U.data());
        }
        if (rc_ == HSDDP_OK && mc_) { r.extra.resize(cnt); rc_ = hsddp_mc_get_extra(s_, 0, batch_, r.extra.data()); }
        if (rc_ == HSDDP_OK && grf_run_) {
            r.grf.resize(cnt); if (keep_) r.Y.resize(cnt * (size_t)n_ * 12);
            rc_ = hsddp_grf_get(s_, 0, batch_, r.grf.data(), keep_ ? r.Y.data() : nullptr);
        }
        return r;
    }
    const double* device_final() { return s_ ? hsddp_sim_device_final(s_) : nullptr; }      // batch x n_samples x 36 on the device
    int last_error() const { return rc_; }
private:
    hsddp_sim_t* s_ = nullptr;
    int batch_, R_, n_, rc_ = 0; bool keep_, mc_ = false, grf_ = false, grf_run_ = false;      // grf_run_: the last run was made with the records on
};

// Batched closed-loop MPC episodes (include/hsddp_episode.h): one device object on a solver's handle that executes the first n_exec knots of the
// current policy from its own states, commits the tick and hands the states to the next solve on the device.  Survives
// MultiPhaseDDP::reconfigure (advance() rebinds the step map); destroy it before the solver.
struct EpisodeLog { std::vector<double> X, U, Y; };      // batch x (max_ticks n_exec + 1) x 36, batch x max_ticks n_exec x 12 twice
class Episode {
public:
    Episode(hsddp_handle_t* h, int batch, int n_exec, int max_ticks, bool keep_log = false) : batch_(batch), n_(n_exec), ticks_(max_ticks), keep_(keep_log) {
        rc_ = hsddp_episode_create(h, n_exec, max_ticks, keep_log ? 1 : 0, &e_);
        if (rc_ != HSDDP_OK) e_ = nullptr;
    }
    ~Episode() { if (e_) hsddp_episode_destroy(e_); }
    Episode(const Episode&) = delete;
    Episode& operator=(const Episode&) = delete;
    // x0: batch x 36 (host memory, or device memory with src_device = 1): the states of tick 0 and the solver's initial condition
    bool reset(const double* x0, int src_device = 0) { rc_ = e_ ? hsddp_episode_reset(e_, x0, src_device) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // one tick; dist null: the plain walk.  kick: batch x 36 or null, added at step dist->kick_step of the tick
    bool advance(const hsddp_mc_dist_t* dist = nullptr, const double* kick = nullptr, int kick_device = 0) {
        rc_ = e_ ? hsddp_episode_advance(e_, dist, kick, kick_device) : HSDDP_EINVAL; return rc_ == HSDDP_OK;
    }
    // contact-force records for every later tick (include/hsddp_grf.h)
    bool set_grf(double mu, double fz_min = 0.0) { rc_ = e_ ? hsddp_grf_set(hsddp_episode_sim(e_), mu, fz_min) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // sub-stepped integration for every later tick (include/hsddp_substep.h)
    bool set_substeps(int substeps) { rc_ = e_ ? hsddp_substep_set(hsddp_episode_sim(e_), substeps) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // unilateral ground contact for every later tick; the free feet are carried from tick to tick (include/hsddp_contact.h)
    bool set_contact(bool on, double fz_rel = 0.0, double z_ground = 0.0) { rc_ = e_ ? hsddp_contact_set(hsddp_episode_sim(e_), on ? 1 : 0, fz_rel, z_ground) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // Coulomb friction for every later tick; a robot's sliding feet and their lagged normal forces are carried from tick to tick (include/hsddp_friction.h)
    bool set_friction(bool on, const hsddp_friction_t* f = nullptr, const double* mu = nullptr, const int* mu_of = nullptr) { rc_ = e_ ? hsddp_friction_set(hsddp_episode_sim(e_), on ? 1 : 0, f, mu, mu_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // the friction rows of the last tick, which has to be one with the contact rule and friction on
    std::vector<hsddp_friction_row_t> friction() {
        std::vector<hsddp_friction_row_t> r((size_t)batch_);
        rc_ = e_ ? hsddp_friction_get(hsddp_episode_sim(e_), 0, batch_, r.data()) : HSDDP_EINVAL;
        return r;
    }
    // terrain and early touchdown for every later tick; the swing feet a robot holds are carried from tick to tick (include/hsddp_terrain.h)
    bool set_terrain(bool on, const hsddp_terrain_t* t = nullptr, const double* H = nullptr, const int* map_of = nullptr) { rc_ = e_ ? hsddp_terrain_set(hsddp_episode_sim(e_), on ? 1 : 0, t, H, map_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // terrain-aware planning (include/hsddp_touchdown.h): the touchdown heights of the handle's current window from the terrain this episode simulates
    // on; after the window moved (reconfigure, set_references) and before the solve
    bool plan_terrain() { rc_ = e_ ? hsddp_episode_plan_terrain(e_) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // friction-aware planning (include/hsddp_limits.h): mu of every robot's limits row <- kappa * mu_s of the friction row it is simulated on
    bool plan_friction(double kappa = 1.0) { rc_ = e_ ? hsddp_episode_plan_friction(e_, kappa) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // a plant row per robot for the whole episode (include/hsddp_plant.h): plant_of [batch] or null
    bool set_plant(bool on, int n_plants = 0, const double* P = nullptr, const int* plant_of = nullptr) { rc_ = e_ ? hsddp_plant_set(hsddp_episode_sim(e_), on ? 1 : 0, n_plants, P, plant_of) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // per-robot policy latency for every later tick (include/hsddp_latency.h): delay_of [batch] in control steps, or null and one delay for all
    bool set_latency(bool on, const int* delay_of = nullptr, int delay = 0) { rc_ = e_ ? hsddp_latency_set(e_, on ? 1 : 0, delay_of, delay) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    // the delays and the stale steps executed so far
    std::vector<hsddp_latency_row_t> latency() {
        std::vector<hsddp_latency_row_t> r((size_t)batch_);
        rc_ = e_ ? hsddp_latency_get(e_, 0, batch_, r.data()) : HSDDP_EINVAL;
        return r;
    }
    std::vector<hsddp_episode_row_t> rows(std::vector<double>* x_now = nullptr) {
        std::vector<hsddp_episode_row_t> r((size_t)batch_);
        if (x_now) x_now->resize((size_t)batch_ * 36);
        rc_ = e_ ? hsddp_episode_get_rows(e_, 0, batch_, r.data(), x_now ? x_now->data() : nullptr) : HSDDP_EINVAL;
        return r;
    }
    EpisodeLog log() {
        EpisodeLog l;
        if (!e_ || !keep_) { rc_ = HSDDP_EINVAL; return l; }
        const size_t n = (size_t)ticks_ * n_;
        l.X.resize((size_t)batch_ * (n + 1) * 36); l.U.resize((size_t)batch_ * n * 12); l.Y.resize((size_t)batch_ * n * 12);
        rc_ = hsddp_episode_get_log(e_, 0, batch_, l.X.data(), l.U.data(), l.Y.data());
        return l;
    }
    const double* state() { return e_ ? hsddp_episode_device_state(e_) : nullptr; }      // batch x 36 on the device
    bool status(int* tick, int* n_alive, int* n_impacts) { rc_ = e_ ? hsddp_episode_status(e_, tick, n_alive, n_impacts) : HSDDP_EINVAL; return rc_ == HSDDP_OK; }
    int last_error() const { return rc_; }
private:
    hsddp_episode_t* e_ = nullptr;
    int batch_, n_, ticks_, rc_ = 0; bool keep_;
};

template <typename T = double>
class MultiPhaseDDP {
    static_assert(sizeof(T) == sizeof(double), "the reference instantiates double only (MultiPhaseDDP.cpp:562)");
public:
    explicit MultiPhaseDDP(int batch = 1, int device = 0) : batch_(batch), device_(device) {}
    ~MultiPhaseDDP() { if (h_) hsddp_destroy(h_); }
    MultiPhaseDDP(const MultiPhaseDDP&) = delete;
    MultiPhaseDDP& operator=(const MultiPhaseDDP&) = delete;

    // set_multiPhaseProblem (MultiPhaseDDP.h:33-41): also resets the cost / violation trackers (new handle).
    void set_multiPhaseProblem(const std::vector<hsddp_phase_desc_t>& phases_in, const hsddp_model_param_t* mp = nullptr) {
        if (h_) { hsddp_destroy(h_); h_ = nullptr; }
        n_phases = (int)phases_in.size();
        rc_ = hsddp_create(&h_, n_phases, phases_in.data(), mp, batch_, device_);
        if (rc_ == HSDDP_OK && !x0_.empty()) rc_ = hsddp_set_initial_condition(h_, x0_.data());
    }
    // set_initial_condition (MultiPhaseDDP.h:43): x0 is batch x n0 (one row per ensemble member)
    void set_initial_condition(const std::vector<T>& x0_in) { x0_ = x0_in; if (h_) rc_ = hsddp_set_initial_condition(h_, x0_.data()); }
    // what the builders write into Trajectory::Xbar / Ubar before solve (MHPCProblem.cpp:186-193)
    void set_nominal(int phase, const T* Xbar, const T* Ubar, bool per_problem = false) { rc_ = hsddp_set_nominal(h_, phase, Xbar, Ubar, per_problem ? 1 : 0); }

    void solve(HSDDP_OPTION& option, const float& max_cputime = 1e6) { rc_ = hsddp_solve(h_, &option, max_cputime); refresh(); }

    // public step methods (MultiPhaseDDP.h:51-75)
    bool hybrid_rollout(T eps, HSDDP_OPTION& option) { rc_ = hsddp_hybrid_rollout(h_, eps, &option); return rc_ == HSDDP_OK; }
    void linear_rollout(T eps, HSDDP_OPTION& option) { rc_ = hsddp_linear_rollout(h_, eps, &option); }
    void compute_cost(const HSDDP_OPTION& option) { rc_ = hsddp_compute_cost(h_, &option); }
    void LQ_approximation(HSDDP_OPTION& option) { rc_ = hsddp_LQ_approximation(h_, &option); }
    std::vector<int> backward_sweep(T regularization) { std::vector<int> ok(batch_); rc_ = hsddp_backward_sweep(h_, regularization, ok.data()); return ok; }
    void update_nominal_trajectory() { rc_ = hsddp_update_nominal_trajectory(h_); }

    // getters (MultiPhaseDDP.h:77-93), per problem b of the batch
    T get_actual_cost(int b = 0) const { return info_.at(b).actual_cost; }
    T get_dyn_infeasibility(int b = 0) const { return info_.at(b).dyn_feas; }
    T get_path_constraint_violation(int b = 0) const { return info_.at(b).max_pconstr; }
    T get_terminal_constraint_violation(int b = 0) const { return info_.at(b).max_tconstr; }
    void get_solver_info(int& n_iters, int& n_ls_iters, int& n_reg_iters, float& solve_time, int b = 0) const {
        n_iters = info_.at(b).n_iters; n_ls_iters = info_.at(b).n_ls_iters; n_reg_iters = info_.at(b).n_reg_iters; solve_time = hsddp_get_solve_time_ms(h_);
    }
    // the history overload (MultiPhaseDDP.h:85): cost / dynamics feasibility / terminal / path constraint violation after the initial
    // rollout and after every completed inner iteration
    void get_solver_info(std::vector<float>& cost, std::vector<float>& dyn_feas, std::vector<float>& eqn_feas, std::vector<float>& ineq_feas, int b = 0) {
        int n = 0; rc_ = hsddp_get_history(h_, b, 0, nullptr, nullptr, nullptr, nullptr, &n);
        cost.assign(n, 0.f); dyn_feas.assign(n, 0.f); eqn_feas.assign(n, 0.f); ineq_feas.assign(n, 0.f);
        if (rc_ == HSDDP_OK && n > 0) rc_ = hsddp_get_history(h_, b, n, cost.data(), dyn_feas.data(), eqn_feas.data(), ineq_feas.data(), &n);
    }
    int status(int b = 0) const { return info_.at(b).status; }

    // results live in the handle (the reference mutates caller-owned Trajectory objects in place); copy a field out
    std::vector<T> get_field(int phase, hsddp_field f, int b0 = 0, int nb = 1) const {
        int count = 0, elems = 0; hsddp_field_shape(h_, phase, f, &count, &elems);
        std::vector<T> out((size_t)nb * count * elems);
        if (!out.empty()) hsddp_get_field(h_, phase, f, b0, nb, out.data());
        return out;
    }
    int last_error() const { return rc_; }
    // publish_mpc_cmd (MHPC/MHPCLocomotion.cpp:190-287): the first n_steps control knots of one problem in MHPC_Command_lcmt field order,
    // packed on the device (fp32); the caller copies the rows into its lcm-gen struct
    std::vector<unsigned int> export_mpc_command(int problem, int n_steps, double mpc_time, double dt, const float* status_times = nullptr) {
        std::vector<unsigned int> words(1 + (size_t)n_steps * HSDDP_CMD_WORDS_PER_STEP);
        rc_ = hsddp_export_mpc_command(h_, problem, n_steps, mpc_time, dt, status_times, words.data());
        return words;
    }
    // update_foot_placement + publish_mpc_cmd (HKDMPC/HKDMPC.cpp:207-297) of an HKD window: the hkd_command_lcmt row of one problem
    // (include/hsddp_hkd.h; the caller memcpys it into its lcm-gen struct).  status_times: n_phases x 4 contact durations
    // (HkdProblemData::Row::dur), pf_in: the problem's current footholds (hkd_data_lcmt foot_placements), both optional.  libhsddp_hip.so only.
    std::vector<unsigned int> export_hkd_command(int problem, int n_steps, double mpc_time, double dt, const double* status_times = nullptr,
                                                 const float* pf_in = nullptr) {
        std::vector<unsigned int> words(HSDDP_HKD_CMD_WORDS);
        rc_ = hsddp_export_hkd_command(h_, problem, n_steps, mpc_time, dt, status_times, pf_in, words.data());
        return words;
    }
    // the rows of problems [b0, b0+nb) in one launch into `out` (nb x HSDDP_HKD_CMD_WORDS words; device memory when dst_device = 1)
    void export_hkd_commands(int b0, int nb, int n_steps, double mpc_time, double dt, const double* status_times, const float* pf_in,
                             unsigned int* out, int dst_device = 0) {
        rc_ = hsddp_export_hkd_commands(h_, b0, nb, n_steps, mpc_time, dt, status_times, pf_in, out, dst_device);
    }
    // per-problem tracking references of one phase (include/hsddp_refs.h): problems [b0, b0+nb) take `refs` (each [nb][h+1][width], NULL fields
    // keep their values; device memory when src_device = 1).  hsddp_reconfigure returns the window to the shared references: call again after it.
    void set_references(int phase, int b0, int nb, const hsddp_refs_t& refs, int src_device = 0) {
        rc_ = hsddp_set_references(h_, phase, b0, nb, &refs, src_device);
    }
    // the references problems [b0, b0+nb) of a phase track, into host arrays of the same layout (NULL skips a field)
    void get_references(int phase, int b0, int nb, double* xr, double* ur, double* yr, double* foot_pos, double* foot_vel, double* body_pos,
                        int* ref_contact) {
        rc_ = hsddp_get_references(h_, phase, b0, nb, xr, ur, yr, foot_pos, foot_vel, body_pos, ref_contact);
    }
    // per-problem, per-foot touchdown heights (include/hsddp_touchdown.h): heights [nb][4] by leg FL FR HL HR for problems [b0, b0+nb) of a whole-body
    // phase (host memory, or device memory with src_device); touchdown: the heights in use and the stored constraint values (NaN for legs without a
    // touchdown), NULL skips; clear: back to the descriptor's ground_height (-1: every phase); plan_terrain: the heights of the whole window from a
    // terrain grid H [n_maps][ny][nx] at the reference footholds, map_of [batch] or null.
    bool set_touchdown_heights(int phase, const double* heights, int nb, int b0 = 0, bool src_device = false) {
        rc_ = hsddp_touchdown_set(h_, phase, b0, nb, heights, src_device ? 1 : 0); return rc_ == HSDDP_OK;
    }
    bool touchdown(int phase, double* heights, double* values, int b0, int nb) { rc_ = hsddp_touchdown_get(h_, phase, b0, nb, heights, values); return rc_ == HSDDP_OK; }
    bool clear_touchdown_heights(int phase = -1) { rc_ = hsddp_touchdown_clear(h_, phase); return rc_ == HSDDP_OK; }
    bool plan_terrain(const hsddp_terrain_t& t, const double* H, const int* map_of = nullptr, double z_ground = 0.0, bool src_device = false) {
        rc_ = hsddp_touchdown_from_terrain(h_, &t, H, map_of, z_ground, src_device ? 1 : 0); return rc_ == HSDDP_OK;
    }
    // per-problem cost-weight scales (include/hsddp_weights.h): scales [nb][84] = sq[36] | sr[12] | sqf[36] for problems [b0, b0+nb) (host memory, or
    // device memory with src_device) - in every whole-body phase problem b plans with q * sq, r * sr and qf * sqf; they stay across reconfigure.
    // weight_scales: the rows in use (ones when none are set); clear: the kernels of a handle that never had scales.
    bool set_weight_scales(const double* scales, int nb, int b0 = 0, bool src_device = false) {
        rc_ = hsddp_weights_set(h_, b0, nb, scales, src_device ? 1 : 0); return rc_ == HSDDP_OK;
    }
    bool weight_scales(double* scales, int b0, int nb) { rc_ = hsddp_weights_get(h_, b0, nb, scales); return rc_ == HSDDP_OK; }
    bool clear_weight_scales() { rc_ = hsddp_weights_clear(h_); return rc_ == HSDDP_OK; }
    // per-problem constraint limits (include/hsddp_limits.h): rows [nb][12] = torque_limit | joint_lb[3] | joint_ub[3] | h_min | mu | jointspeed_lb |
    // jointspeed_ub | pad for problems [b0, b0+nb), absolute values, NaN = the descriptor's (host memory, or device memory with src_device); they stay
    // across reconfigure.  limits: the rows in use in a phase; clear: the kernels of a handle that never had limits.
    bool set_limits(const double* rows, int nb, int b0 = 0, bool src_device = false) {
        rc_ = hsddp_limits_set(h_, b0, nb, rows, src_device ? 1 : 0); return rc_ == HSDDP_OK;
    }
    bool limits(double* rows, int phase, int b0, int nb) { rc_ = hsddp_limits_get(h_, phase, b0, nb, rows); return rc_ == HSDDP_OK; }
    bool clear_limits() { rc_ = hsddp_limits_clear(h_); return rc_ == HSDDP_OK; }
    // one-off closed-loop rollouts of the current policy, u = Ubar + K (x - Xbar), from n_samples initial states per problem over the first
    // n_steps whole-body control knots (x0: batch x n_samples x 36) - what the controller side of the reference does one state at a time
    // (MHPC/MHPC-Trajopt/test/testTrajOptInLoop.cpp).  An MPC loop keeps a hsddp::Simulation instead.  libhsddp_hip.so only.
    SimResult simulate(const T* x0, int n_samples, int n_steps, bool keep_traj = false, int src_device = 0) {
        Simulation sim(h_, batch_, n_samples, n_steps, keep_traj);
        SimResult r;
        if (sim.last_error() == HSDDP_OK && sim.run(x0, src_device)) r = sim.result();
        rc_ = sim.last_error();
        return r;
    }
    // receding-horizon step (MHPCProblem::update): phase `dphase` continues phase `sphase` of the previous window (sphase < 0: new phase)
    void warm_start_phase(int dphase, MultiPhaseDDP<T>* prev, int sphase, int popped_front) {
        rc_ = hsddp_warm_start_phase(h_, dphase, prev ? prev->h_ : nullptr, sphase, popped_front);
    }
    // receding-horizon step INSIDE the handle (what MHPCLocomotion::update gets from MHPCProblem::update + a new solver object,
    // MHPC/MHPCLocomotion.cpp:102-122): new phase table, trajectories and constraint parameters moved device to device, allocations reused
    void reconfigure(const std::vector<hsddp_phase_desc_t>& phases_in, const std::vector<int>& src_phase, const std::vector<int>& shift) {
        n_phases = (int)phases_in.size();
        rc_ = hsddp_reconfigure(h_, n_phases, phases_in.data(), src_phase.data(), shift.data());
    }
    // Trajectory::Ubar[k] written by the caller between solves (HKDProblem::update: Ubar[0].setZero(), HKDProblem.cpp:220); u = nullptr: zeros
    void set_control_knot(int phase, int k, const T* u = nullptr) { rc_ = hsddp_set_control_knot(h_, phase, k, u); }
    // solver_info_lcmt (lcmtypes/solver_info_lcmt.lcm) as MHPCLocomotion fills it after a solve (MHPC/MHPCLocomotion.cpp:74-79)
    struct SolverInfo { int n_iter, n_ls_iter, n_reg_iter; float solve_time, cost, dyn_feas, ineq_violation, eq_violation; };
    SolverInfo export_solver_info(int problem = 0) {
        static_assert(sizeof(SolverInfo) == 4 * HSDDP_SOLVER_INFO_WORDS, "solver_info_lcmt: eight 32-bit fields");
        SolverInfo s{}; rc_ = hsddp_export_solver_info(h_, problem, reinterpret_cast<unsigned int*>(&s)); return s;
    }
    hsddp_handle_t* handle() { return h_; }

private:
    void refresh() { info_.resize(batch_); if (h_) hsddp_get_info(h_, info_.data()); }
    hsddp_handle_t* h_ = nullptr;
    int batch_, device_, n_phases = 0, rc_ = 0;
    std::vector<T> x0_;
    std::vector<hsddp_info_t> info_;
};

}  // namespace hsddp
