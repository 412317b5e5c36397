// Host side of the closed-loop policy simulation and of the MPC episodes: the C entry points of include/hsddp_sim.h, hsddp_mc.h, hsddp_grf.h,
// hsddp_substep.h, hsddp_contact.h, hsddp_terrain.h, hsddp_plant.h, hsddp_friction.h, hsddp_episode.h and hsddp_latency.h.  Part of hsddp_hip.hip's translation unit, host pass only: that
// file includes it inside its host-only region, behind hsddp_handle, HIPCK, Timed and drain_events, which this code uses.  The kernels are those of
// wb_sim.hpp, hsddp_sub.hip, hsddp_uni.hip, hsddp_ter.hip, hsddp_plant.hip, hsddp_fric.hip and episode.hpp; which walk a run launches is sim_pick's business (sim_pick.hpp).
#pragma once
#include "plant_host.hpp"

// One error check for every allocation and copy below whose failure has to tell out-of-memory from the rest: the message of HIPCK, HSDDP_ENOMEM on out
// of memory, else HSDDP_ENODEV.  SIM_CK returns at once and frees nothing: in the set calls and in hsddp_mc_run the buffers made before the failure are
// kept for the next call and freed with the object, and the switch keeps the state it had - "nothing changed" holds for what a run does, not for those
// allocations.  SIM_CK_FREE(x, FREE) runs FREE first: the two create calls, which give back the half-made object.
static int sim_ck_fail(hipError_t e, const char* what, const char* file, int line) {
    fprintf(stderr, "[hsddp_hip] %s failed: %s (%s:%d)\n", what, hipGetErrorString(e), file, line);
    return e == hipErrorOutOfMemory ? HSDDP_ENOMEM : HSDDP_ENODEV;
}
#define SIM_CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return sim_ck_fail(e_, #x, __FILE__, __LINE__); } while (0)
#define SIM_CK_FREE(x, FREE) do { hipError_t e_ = (x); if (e_ != hipSuccess) { const int rc_ = sim_ck_fail(e_, #x, __FILE__, __LINE__); FREE; return rc_; } } while (0)

struct hsddp_sim {
    hsddp_handle* h = nullptr;
    int R = 0, n_steps = 0, keep = 0, gen = 0;
    int* d_map = nullptr;                                  // [3][n_steps] step -> phase, knot, reset map behind the step (wb_sim.hpp)
    double *d_x0 = nullptr, *d_final = nullptr, *d_rows = nullptr, *d_X = nullptr, *d_U = nullptr;      // [B R] x 36 / 36 / SIM_ROW / (n_steps+1) 36 / n_steps 12
    hipEvent_t ev0 = nullptr, ev1 = nullptr; bool timed = false;
    // disturbed runs (hsddp_mc.h): allocated at the first one.  last_mc: 0 the last run was plain, 1 disturbed, 2 hsddp_mc_run with every switch off
    double *d_extra = nullptr, *d_kick = nullptr; WbsMcArgs* d_mc = nullptr;      // [B R][2] first_fall | n_sat ; staging of a host kick ; the switches
    int last_mc = 0;
    // contact-force records (hsddp_grf.h): allocated by the first hsddp_grf_set that switches them on.  grf_on: what later runs do; last_grf: what the last run did
    double *d_grf_rows = nullptr, *d_Y = nullptr; WbsGrfArgs* d_grf = nullptr;      // [B R][SIM_GRF_ROW] ; [B R][n_steps][12] (keep) ; thresholds and destinations
    bool grf_on = false, last_grf = false;
    // sub-stepped integration (hsddp_substep.h): what later runs use; the trip count on the device, allocated by the first hsddp_substep_set above 1
    int substeps = 1; WbsSubArgs* d_sub = nullptr;
    // unilateral ground contact (hsddp_contact.h): everything below is allocated by the first hsddp_contact_set that switches the rule on.
    // uni_on: what later runs do; last_uni: what the last run did.  d_uni_grf / d_uni_grows: thresholds and rows of the records the walk always keeps,
    // used while hsddp_grf_set has them off.  d_uni_F: the free flags an episode carries from tick to tick (uni_keep, set by hsddp_episode_create;
    // uni_hold: the end_reason of the episode's rows, stride in ints)
    bool uni_on = false, last_uni = false, uni_keep = false;
    double uni_fz_rel = 0.0, uni_z_ground = 0.0;
    WbsUniArgs* d_uni = nullptr; double *d_uni_rows = nullptr, *d_uni_F = nullptr, *d_uni_grows = nullptr; WbsGrfArgs* d_uni_grf = nullptr;
    const int* uni_hold = nullptr; int uni_hold_stride = 0;
    // terrain and early touchdown (hsddp_terrain.h): allocated by hsddp_terrain_set calls that switch it on (the grid again when it grows: ter_cap
    // doubles).  ter_on: what later runs ask for - it acts while uni_on is set too; last_ter: the last run launched the _ter kernels.  d_ter_E: the early
    // flags an episode carries from tick to tick (uni_keep), under the hold of d_uni_F
    bool ter_on = false, last_ter = false;
    hsddp_terrain_t ter = {};
    WbsTerArgs* d_ter = nullptr; double *d_ter_H = nullptr, *d_ter_rows = nullptr, *d_ter_E = nullptr; int* d_ter_map = nullptr; size_t ter_cap = 0;
    // per-sample plant (hsddp_plant.h): allocated by hsddp_plant_set calls that switch it on (the table again when it grows: plant_cap rows).  plant_on:
    // what later runs do.  plant_rows: the host's copy of the table, for hsddp_plant_get_table.  The _plant walks always keep the force records and read
    // the trip count from the device: while hsddp_grf_set has the records off they go to d_uni_grows through d_uni_grf (the buffer the walks with the
    // contact rule use for the same purpose), and d_sub is made current by the set call as hsddp_contact_set does
    bool plant_on = false; int n_plants = 0;
    WbsPlantArgs* d_plant = nullptr; double* d_plant_P = nullptr; int* d_plant_of = nullptr; size_t plant_cap = 0;
    std::vector<double> plant_rows;
    // Coulomb friction (hsddp_friction.h): allocated by hsddp_friction_set calls that switch it on (the table again when it grows: fric_cap rows).  fric_on:
    // what later runs ask for - it acts while uni_on is set too; last_fric: the last run launched the _fric kernels.  d_fric_Sl / d_fric_NF: the sliding
    // flags and lagged normal forces an episode carries from tick to tick (uni_keep), under the hold of d_uni_F.  d_fric_ter: the one-cell flat map without
    // early touchdown the _fric kernels are given while the terrain is off (d_fric_H its cell, d_fric_tmap its all-zero index, d_fric_trows its unread rows)
    bool fric_on = false, last_fric = false;
    hsddp_friction_t fric = {};
    WbsFricArgs* d_fric = nullptr; double *d_fric_mu = nullptr, *d_fric_rows = nullptr, *d_fric_Sl = nullptr, *d_fric_NF = nullptr; int* d_fric_of = nullptr; size_t fric_cap = 0;
    WbsTerArgs* d_fric_ter = nullptr; double *d_fric_H = nullptr, *d_fric_trows = nullptr; int* d_fric_tmap = nullptr;
    // policy latency of an episode (hsddp_latency.h): the descriptor table and the step map the NEXT launch walks instead of h->d_ph and d_map, set
    // by hsddp_episode_advance around its walk and null otherwise
    const PhaseDev* walk_ph = nullptr; const int* walk_map = nullptr;
};
static void sim_free(hsddp_sim* s) {
    if (!s) return;
    hipSetDevice(s->h->device);
    if (s->h->stream) hipStreamSynchronize(s->h->stream);
    void* p[] = {s->d_map, s->d_x0, s->d_final, s->d_rows, s->d_X, s->d_U, s->d_extra, s->d_kick, s->d_mc, s->d_grf_rows, s->d_Y, s->d_grf, s->d_sub, s->d_uni, s->d_uni_rows, s->d_uni_F, s->d_uni_grows, s->d_uni_grf,
                 s->d_ter, s->d_ter_H, s->d_ter_rows, s->d_ter_E, s->d_ter_map, s->d_plant, s->d_plant_P, s->d_plant_of,
                 s->d_fric, s->d_fric_mu, s->d_fric_rows, s->d_fric_Sl, s->d_fric_NF, s->d_fric_of, s->d_fric_ter, s->d_fric_H, s->d_fric_trows, s->d_fric_tmap};
    for (void* q : p) if (q) hipFree(q);
    if (s->ev0) hipEventDestroy(s->ev0);
    if (s->ev1) hipEventDestroy(s->ev1);
    delete s;
}
static bool sim_range_ok(const hsddp_sim* s, int b0, int nb) { return s && nb > 0 && b0 >= 0 && b0 <= s->h->batch - nb; }
// step -> (phase, knot) over the leading whole-body control knots of the handle's CURRENT window, as hsddp_export_mpc_command walks them; the reset
// map of a phase is applied behind its last knot when the window goes on.  map: 3 n_steps ints.  False if the window holds fewer such knots.
// pending (optional): the phase whose reset map lies behind the LAST step - the one no run applies (hsddp_episode.h) - or -1.
static bool sim_step_map(const hsddp_handle* h, int n_steps, int* map, int* pending = nullptr) {
    int n = 0, pend = -1;
    for (int i = 0; i < h->nph && n < n_steps; i++) {
        if (h->ph[i].model != HSDDP_MODEL_WB) break;
        for (int k = 0; k < h->ph[i].h && n < n_steps; k++, n++) {
            map[n] = i; map[n_steps + n] = k;
            const bool td = k == h->ph[i].h - 1 && h->ph[i].has_impact;
            map[2 * (size_t)n_steps + n] = (td && n + 1 < n_steps) ? 1 : 0;
            if (td && n + 1 == n_steps) pend = i;
        }
    }
    if (pending) *pending = pend;
    return n == n_steps;
}
// the switches hsddp_mc_run accepts on object s
static bool mc_dist_ok(const hsddp_sim* s, const hsddp_mc_dist_t* d, const double* kick) {
    auto sigma_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!sigma_ok(d->sigma_u) || !sigma_ok(d->sigma_q) || !sigma_ok(d->sigma_v) || !std::isfinite(d->u_max) || !std::isfinite(d->fall_height) || d->first_problem < 0) return false;
    if (kick && (d->kick_step < 0 || d->kick_step >= s->n_steps)) return false;
    return s->n_steps <= 65536 && s->R <= 65536;      // the generator numbers samples and steps in 16 bits each
}
// The samples of problems [b0, b0 + nb) of a per-sample table of w doubles a row, fetched to the host; unpack(i, q) gets sample i of the range and its row.
template <class F> static int sim_fetch_rows(hsddp_sim* s, int b0, int nb, const double* d_table, int w, F unpack) {
    HIPCK(hipSetDevice(s->h->device));
    const size_t cnt = (size_t)nb * s->R, off = (size_t)b0 * s->R;
    std::vector<double> r(cnt * w);
    HIPCK(hipMemcpy(r.data(), d_table + off * w, r.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cnt; i++) unpack(i, &r[i * w]);
    return HSDDP_OK;
}
// What the walks that always keep the force records and always run the sub-step loop need beside their own blocks (hsddp_contact_set, hsddp_plant_set): the
// dummy records d_uni_grf -> d_uni_grows, used while hsddp_grf_set has the records off, and the trip count on the device.
static int sim_ensure_records_and_trip_count(hsddp_sim* s) {
    hsddp_handle* h = s->h;
    const size_t total = (size_t)h->batch * s->R;
    if (!s->d_uni_grows) SIM_CK(hipMalloc((void**)&s->d_uni_grows, total * SIM_GRF_ROW * 8));
    if (!s->d_uni_grf) {
        SIM_CK(hipMalloc((void**)&s->d_uni_grf, sizeof(WbsGrfArgs)));
        WbsGrfArgs g;
        g.mu = 1.0; g.fz_min = 0.0; g.rows = s->d_uni_grows; g.Y = nullptr;      // (nobody reads these records: hsddp_grf_get refuses while the records are off)
        HIPCK(hipMemcpyAsync(s->d_uni_grf, &g, sizeof(g), hipMemcpyHostToDevice, h->stream));
    }
    if (!s->d_sub) {      // the walk reads its trip count from here for S = 1 too; from now on hsddp_substep_set keeps it current
        SIM_CK(hipMalloc((void**)&s->d_sub, sizeof(WbsSubArgs)));
        WbsSubArgs b;
        b.substeps = s->substeps; b.pad = 0;
        HIPCK(hipMemcpyAsync(s->d_sub, &b, sizeof(b), hipMemcpyHostToDevice, h->stream));
    }
    return HSDDP_OK;
}
// A device table of doubles that only grows (the terrain grid, the plant table): room for `need` units of `unit` doubles.  The new block first, so that a
// failure leaves the old one in place.
static int sim_grow(hsddp_handle* h, double*& d_table, size_t& cap, size_t need, size_t unit) {
    if (need <= cap) return HSDDP_OK;
    double* nb = nullptr;
    SIM_CK(hipMalloc((void**)&nb, need * unit * 8));
    HIPCK(hipStreamSynchronize(h->stream));
    if (d_table) hipFree(d_table);
    d_table = nb; cap = need;
    return HSDDP_OK;
}

// (hsddp_friction.h) friction and the per-sample plant would both act in the next run: every entry point that starts one - hsddp_sim_run, hsddp_mc_run,
// hsddp_episode_advance - asks this FIRST and answers HSDDP_ENOTSUP before it allocates, copies or launches anything (the rule itself is sim_pick's)
static bool sim_unsupported(const hsddp_sim* s) { return sim_pick(SimSwitches{s->plant_on, s->uni_on, s->ter_on, s->substeps, s->grf_on, false, false, s->fric_on}).unsupported; }

extern "C" {

int hsddp_sim_create(hsddp_handle_t* h, int n_samples, int n_steps, int keep_traj, hsddp_sim_t** out) {
    if (!h || !out || n_samples <= 0 || n_steps <= 0) return HSDDP_EINVAL;
    std::vector<int> map(3 * (size_t)n_steps, 0);
    if (!sim_step_map(h, n_steps, map.data())) return HSDDP_EINVAL;
    const size_t total = (size_t)h->batch * n_samples;
    if (total >= ((size_t)1 << 31)) return HSDDP_ENOTSUP;      // quads are indexed in 32 bits
    HIPCK(hipSetDevice(h->device));
    hsddp_sim* s = new hsddp_sim();
    s->h = h; s->R = n_samples; s->n_steps = n_steps; s->keep = keep_traj ? 1 : 0; s->gen = h->window_gen;
    SIM_CK_FREE(hipMalloc((void**)&s->d_map, map.size() * sizeof(int)), sim_free(s));
    SIM_CK_FREE(hipMalloc((void**)&s->d_x0, total * 36 * 8), sim_free(s));
    SIM_CK_FREE(hipMalloc((void**)&s->d_final, total * 36 * 8), sim_free(s));
    SIM_CK_FREE(hipMalloc((void**)&s->d_rows, total * SIM_ROW * 8), sim_free(s));
    if (s->keep) { SIM_CK_FREE(hipMalloc((void**)&s->d_X, total * (n_steps + 1) * 36 * 8), sim_free(s)); SIM_CK_FREE(hipMalloc((void**)&s->d_U, total * n_steps * 12 * 8), sim_free(s)); }
    SIM_CK_FREE(hipEventCreate(&s->ev0), sim_free(s)); SIM_CK_FREE(hipEventCreate(&s->ev1), sim_free(s));
    SIM_CK_FREE(hipMemcpy(s->d_map, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice), sim_free(s));
    SIM_CK_FREE(hipMemset(s->d_final, 0, total * 36 * 8), sim_free(s)); SIM_CK_FREE(hipMemset(s->d_rows, 0, total * SIM_ROW * 8), sim_free(s));
    *out = s; return HSDDP_OK;
}

void hsddp_sim_destroy(hsddp_sim_t* s) { sim_free(s); }

// the one launch path of a run.  mc: a disturbed run, its switches already on the device at s->d_mc (noise: with the generator).  The launch record names
// the common arguments once, sim_pick (sim_pick.hpp) chooses the walk from the object's switches and the run's, and the family's launcher launches it.
static int sim_launch(hsddp_sim* s, const double* x0, int src_device, bool mc, bool noise = false) {
    hsddp_handle* h = s->h;
    const size_t total = (size_t)h->batch * s->R;
    const SimPick pick = sim_pick(SimSwitches{s->plant_on, s->uni_on, s->ter_on, s->substeps, s->grf_on, mc, noise, s->fric_on});
    if (pick.unsupported) return HSDDP_ENOTSUP;      // (the entry points have asked sim_unsupported already; kept for a caller that does not)
    if (!src_device) HIPCK(hipMemcpyAsync(s->d_x0, x0, total * 36 * 8, hipMemcpyHostToDevice, h->stream));
    HIPCK(hipEventRecord(s->ev0, h->stream));
    WbsLaunch L;
    L.stream = h->stream; L.grid = (unsigned)((total + 15) / 16);
    L.ph = s->walk_ph ? s->walk_ph : h->d_ph; L.md = &h->md; L.map = s->walk_map ? s->walk_map : s->d_map; L.n_steps = s->n_steps; L.n_samples = s->R; L.total = (int)total;
    L.x0 = src_device ? x0 : s->d_x0; L.xfinal = s->d_final; L.rows = s->d_rows; L.trajX = s->d_X; L.trajU = s->d_U;
    L.pick = pick;
    L.mc = s->d_mc; L.gr = L.pick.records ? s->d_grf : s->d_uni_grf; L.sb = s->d_sub; L.un = s->d_uni; L.te = s->d_ter; L.pl = s->d_plant;
    if (L.pick.family == SIM_FAM_FRIC) { L.fc = s->d_fric; if (L.pick.contact != SIM_TERRAIN) L.te = s->d_fric_ter; }      // (terrain off: the flat map)
    switch (L.pick.family) {      // (the launchers leave the runtime's error state alone: a failed launch is caught by the hipGetLastError below)
        case SIM_FAM_BASE: wbs_base_launch(L); break;
        case SIM_FAM_SUB: wbs_sub_launch(L); break;
        case SIM_FAM_UNI: wbs_uni_launch(L); break;
        case SIM_FAM_TER: wbs_ter_launch(L); break;
        case SIM_FAM_PLANT: wbs_plant_launch(L); break;
        case SIM_FAM_FRIC: wbs_fric_launch(L); break;
    }
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(s->ev1, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    s->timed = true; s->last_grf = s->grf_on; s->last_uni = s->uni_on; s->last_ter = L.pick.contact == SIM_TERRAIN; s->last_fric = L.pick.family == SIM_FAM_FRIC;
    return HSDDP_OK;
}

int hsddp_sim_run(hsddp_sim_t* s, const double* x0, int src_device) {
    if (!s || !x0) return HSDDP_EINVAL;
    hsddp_handle* h = s->h;
    if (s->gen != h->window_gen) return HSDDP_EINVAL;      // hsddp_reconfigure moved the window: the step map is that of the old one
    if (sim_unsupported(s)) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    const int rc = sim_launch(s, x0, src_device, false);
    if (rc == HSDDP_OK) s->last_mc = 0;
    return rc;
}

int hsddp_mc_run(hsddp_sim_t* s, const double* x0, int x0_device, const hsddp_mc_dist_t* d, const double* kick, int kick_device) {
    if (!s || !x0 || !d) return HSDDP_EINVAL;
    hsddp_handle* h = s->h;
    if (s->gen != h->window_gen) return HSDDP_EINVAL;
    if (!mc_dist_ok(s, d, kick)) return HSDDP_EINVAL;
    if (sim_unsupported(s)) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    if (!kick && d->sigma_u == 0.0 && d->sigma_q == 0.0 && d->sigma_v == 0.0 && d->u_max <= 0.0 && d->fall_height <= 0.0) {      // nothing switched on: the plain kernel
        const int rc = sim_launch(s, x0, x0_device, false);
        if (rc == HSDDP_OK) s->last_mc = 2;
        return rc;
    }
    const size_t total = (size_t)h->batch * s->R;
    if (!s->d_extra) SIM_CK(hipMalloc((void**)&s->d_extra, total * 2 * 8));
    if (!s->d_mc) SIM_CK(hipMalloc((void**)&s->d_mc, sizeof(WbsMcArgs)));
    if (kick && !kick_device && !s->d_kick) SIM_CK(hipMalloc((void**)&s->d_kick, total * 36 * 8));
    if (kick && !kick_device) HIPCK(hipMemcpyAsync(s->d_kick, kick, total * 36 * 8, hipMemcpyHostToDevice, h->stream));
    WbsMcArgs a;
    a.seed = d->seed; a.first_problem = (unsigned long long)d->first_problem;
    a.su = d->sigma_u; a.sq = d->sigma_q; a.sv = d->sigma_v; a.umax = d->u_max; a.fall = d->fall_height;
    a.kick_step = kick ? d->kick_step : -1; a.R = s->R;
    a.kick = kick ? (kick_device ? kick : s->d_kick) : nullptr; a.extra = s->d_extra;
    HIPCK(hipMemcpyAsync(s->d_mc, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));      // (pageable source: staged before the call returns)
    const int rc = sim_launch(s, x0, x0_device, true, d->sigma_u > 0.0 || d->sigma_q > 0.0 || d->sigma_v > 0.0);      // (without noise: the walk compiled without the generator)
    if (rc == HSDDP_OK) s->last_mc = 1;
    return rc;
}

int hsddp_mc_get_extra(hsddp_sim_t* s, int b0, int nb, hsddp_mc_extra_t* out) {
    if (!sim_range_ok(s, b0, nb) || !out || s->last_mc == 0) return HSDDP_EINVAL;
    if (s->last_mc == 2) { for (size_t i = 0, cnt = (size_t)nb * s->R; i < cnt; i++) { out[i].first_fall = -1; out[i].n_sat = 0; } return HSDDP_OK; }
    return sim_fetch_rows(s, b0, nb, s->d_extra, 2, [&](size_t i, const double* q) { out[i].first_fall = (int)q[0]; out[i].n_sat = (int)q[1]; });
}

int hsddp_sim_get_rows(hsddp_sim_t* s, int b0, int nb, hsddp_sim_row_t* rows, double* x_final) {
    if (!sim_range_ok(s, b0, nb) || !rows) return HSDDP_EINVAL;
    const int rc = sim_fetch_rows(s, b0, nb, s->d_rows, SIM_ROW, [&](size_t i, const double* q) {
        rows[i].dev_q = q[0]; rows[i].dev_v = q[1]; rows[i].min_height = q[2]; rows[i].max_torque = q[3]; rows[i].first_bad = (int)q[4]; rows[i].pad = 0;
    });
    if (rc != HSDDP_OK) return rc;
    const size_t cnt = (size_t)nb * s->R, off = (size_t)b0 * s->R;
    if (x_final) HIPCK(hipMemcpy(x_final, s->d_final + off * 36, cnt * 36 * 8, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_sim_get_traj(hsddp_sim_t* s, int b0, int nb, double* X, double* U) {
    if (!sim_range_ok(s, b0, nb) || !s->keep) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(s->h->device));
    const size_t cnt = (size_t)nb * s->R, off = (size_t)b0 * s->R, sx = (size_t)(s->n_steps + 1) * 36, su = (size_t)s->n_steps * 12;
    if (X) HIPCK(hipMemcpy(X, s->d_X + off * sx, cnt * sx * 8, hipMemcpyDeviceToHost));
    if (U) HIPCK(hipMemcpy(U, s->d_U + off * su, cnt * su * 8, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_grf_set(hsddp_sim_t* s, double mu, double fz_min) {
    if (!s || !std::isfinite(mu) || !std::isfinite(fz_min) || mu < 0.0 || fz_min < 0.0) return HSDDP_EINVAL;
    if (mu == 0.0) { s->grf_on = false; return HSDDP_OK; }      // later runs launch the kernels without records; the buffers are kept
    hsddp_handle* h = s->h;
    HIPCK(hipSetDevice(h->device));
    const size_t total = (size_t)h->batch * s->R;
    if (!s->d_grf_rows) SIM_CK(hipMalloc((void**)&s->d_grf_rows, total * SIM_GRF_ROW * 8));      // (a failure: see SIM_CK - the records stay off)
    if (s->keep && !s->d_Y) SIM_CK(hipMalloc((void**)&s->d_Y, total * (size_t)s->n_steps * 12 * 8));
    if (!s->d_grf) SIM_CK(hipMalloc((void**)&s->d_grf, sizeof(WbsGrfArgs)));
    WbsGrfArgs a;
    a.mu = mu; a.fz_min = fz_min; a.rows = s->d_grf_rows; a.Y = s->keep ? s->d_Y : nullptr;
    HIPCK(hipMemcpyAsync(s->d_grf, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));      // (pageable source: staged before the call returns; the runs are on this stream)
    s->grf_on = true;
    return HSDDP_OK;
}

int hsddp_grf_get(hsddp_sim_t* s, int b0, int nb, hsddp_grf_row_t* rows, double* Y) {
    if (!sim_range_ok(s, b0, nb) || !rows || !s->last_grf || (Y && !s->keep)) return HSDDP_EINVAL;
    const int rc = sim_fetch_rows(s, b0, nb, s->d_grf_rows, SIM_GRF_ROW, [&](size_t i, const double* q) {
        rows[i].min_fz = q[0]; rows[i].min_cone = q[1]; rows[i].max_fz = q[2]; rows[i].first_slip = (int)q[3]; rows[i].n_slip = (int)q[4];
    });
    if (rc != HSDDP_OK) return rc;
    const size_t cnt = (size_t)nb * s->R, off = (size_t)b0 * s->R, sy = (size_t)s->n_steps * 12;
    if (Y) HIPCK(hipMemcpy(Y, s->d_Y + off * sy, cnt * sy * 8, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_substep_set(hsddp_sim_t* s, int substeps) {
    if (!s || substeps < 1 || substeps > HSDDP_SUBSTEP_MAX) return HSDDP_EINVAL;
    hsddp_handle* h = s->h;
    if (substeps > 1 || s->d_sub) {      // (an object that never asks for more than one holds what it held before)
        HIPCK(hipSetDevice(h->device));
        if (!s->d_sub) {
            hipError_t e_ = hipMalloc((void**)&s->d_sub, sizeof(WbsSubArgs));
            if (e_ != hipSuccess) { fprintf(stderr, "[hsddp_hip] hipMalloc of the substep block failed: %s\n", hipGetErrorString(e_)); s->d_sub = nullptr; return e_ == hipErrorOutOfMemory ? HSDDP_ENOMEM : HSDDP_ENODEV; }
        }
        WbsSubArgs a;
        a.substeps = substeps; a.pad = 0;
        HIPCK(hipMemcpyAsync(s->d_sub, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));      // (pageable source: staged before the call returns; the runs are on this stream)
    }
    s->substeps = substeps;
    return HSDDP_OK;
}

int hsddp_substep_get(hsddp_sim_t* s, int* substeps) {
    if (!s || !substeps) return HSDDP_EINVAL;
    *substeps = s->substeps;
    return HSDDP_OK;
}

int hsddp_contact_set(hsddp_sim_t* s, int on, double fz_rel, double z_ground) {
    if (!s || !std::isfinite(fz_rel) || !std::isfinite(z_ground)) return HSDDP_EINVAL;
    if (!on) { s->uni_on = false; return HSDDP_OK; }      // later runs launch the kernels without the rule; the buffers and the thresholds are kept
    hsddp_handle* h = s->h;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    const size_t total = (size_t)h->batch * s->R;
    if (!s->d_uni) SIM_CK(hipMalloc((void**)&s->d_uni, sizeof(WbsUniArgs)));      // (a failure: see SIM_CK - the rule stays off)
    if (!s->d_uni_rows) SIM_CK(hipMalloc((void**)&s->d_uni_rows, total * SIM_UNI_ROW * 8));
    if (s->uni_keep && !s->d_uni_F) { SIM_CK(hipMalloc((void**)&s->d_uni_F, total * 4 * 8)); HIPCK(hipMemsetAsync(s->d_uni_F, 0, total * 4 * 8, h->stream)); }
    const int rc = sim_ensure_records_and_trip_count(s);
    if (rc != HSDDP_OK) return rc;
    WbsUniArgs a;
    a.fz_rel = fz_rel; a.z_ground = z_ground; a.rows = s->d_uni_rows; a.F = s->d_uni_F; a.hold = s->uni_hold; a.hold_stride = s->uni_hold_stride; a.pad = 0;
    HIPCK(hipMemcpyAsync(s->d_uni, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));      // (pageable sources: staged before the calls return; the runs are on this stream)
    s->uni_on = true; s->uni_fz_rel = fz_rel; s->uni_z_ground = z_ground;
    return HSDDP_OK;
}

int hsddp_contact_get_params(hsddp_sim_t* s, int* on, double* fz_rel, double* z_ground) {
    if (!s || !on || !fz_rel || !z_ground) return HSDDP_EINVAL;
    *on = s->uni_on ? 1 : 0; *fz_rel = s->uni_fz_rel; *z_ground = s->uni_z_ground;
    return HSDDP_OK;
}

int hsddp_contact_get(hsddp_sim_t* s, int b0, int nb, hsddp_contact_row_t* rows) {
    if (!sim_range_ok(s, b0, nb) || !rows || !s->last_uni) return HSDDP_EINVAL;
    return sim_fetch_rows(s, b0, nb, s->d_uni_rows, SIM_UNI_ROW, [&](size_t i, const double* q) {
        rows[i].first_release = (int)q[0]; rows[i].n_release = (int)q[1]; rows[i].n_land = (int)q[2]; rows[i].n_free = (int)q[3]; rows[i].free_final = (int)q[4]; rows[i].pad = 0;
        rows[i].max_lift = q[5];
    });
}

int hsddp_terrain_set(hsddp_sim_t* s, int on, const hsddp_terrain_t* t, const double* H, const int* map_of) {
    if (!s) return HSDDP_EINVAL;
    if (!on) { s->ter_on = false; return HSDDP_OK; }      // later runs launch the kernels without the terrain; the buffers and the parameters are kept
    if (!t || !H) return HSDDP_EINVAL;
    if (!std::isfinite(t->x0) || !std::isfinite(t->y0) || !std::isfinite(t->cx) || !std::isfinite(t->cy) || !std::isfinite(t->w_td)) return HSDDP_EINVAL;
    if (!(t->cx > 0.0) || !(t->cy > 0.0) || t->w_td < 0.0) return HSDDP_EINVAL;
    if (t->nx < 1 || t->nx > 1024 || t->ny < 1 || t->ny > 1024 || t->n_maps < 1 || t->n_maps > 4096) return HSDDP_EINVAL;
    const size_t cells = (size_t)t->n_maps * (size_t)t->nx * (size_t)t->ny;
    if (cells > ((size_t)1 << 22)) return HSDDP_EINVAL;
    for (size_t i = 0; i < cells; i++) if (!std::isfinite(H[i])) return HSDDP_EINVAL;
    hsddp_handle* h = s->h;
    const size_t total = (size_t)h->batch * s->R;
    if (map_of) for (size_t i = 0; i < total; i++) if (map_of[i] < 0 || map_of[i] >= t->n_maps) return HSDDP_EINVAL;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    if (!s->d_ter) SIM_CK(hipMalloc((void**)&s->d_ter, sizeof(WbsTerArgs)));      // (a failure: see SIM_CK - the terrain stays as it was)
    if (!s->d_ter_rows) SIM_CK(hipMalloc((void**)&s->d_ter_rows, total * SIM_TER_ROW * 8));
    if (!s->d_ter_map) SIM_CK(hipMalloc((void**)&s->d_ter_map, total * sizeof(int)));
    if (s->uni_keep && !s->d_ter_E) { SIM_CK(hipMalloc((void**)&s->d_ter_E, total * 4 * 8)); HIPCK(hipMemsetAsync(s->d_ter_E, 0, total * 4 * 8, h->stream)); }
    const int rc = sim_grow(h, s->d_ter_H, s->ter_cap, cells, 1);
    if (rc != HSDDP_OK) return rc;
    HIPCK(hipMemcpyAsync(s->d_ter_H, H, cells * 8, hipMemcpyHostToDevice, h->stream));
    if (map_of) HIPCK(hipMemcpyAsync(s->d_ter_map, map_of, total * sizeof(int), hipMemcpyHostToDevice, h->stream));
    else HIPCK(hipMemsetAsync(s->d_ter_map, 0, total * sizeof(int), h->stream));
    WbsTerArgs a;
    a.H = s->d_ter_H; a.map_of = s->d_ter_map; a.nx = t->nx; a.ny = t->ny; a.n_maps = t->n_maps; a.early = t->early ? 1 : 0;
    a.x0 = t->x0; a.y0 = t->y0; a.cx = t->cx; a.cy = t->cy; a.w_td = t->w_td; a.rows = s->d_ter_rows; a.E = s->d_ter_E;
    HIPCK(hipMemcpyAsync(s->d_ter, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));      // H and map_of are the caller's: they may go once the call returns
    s->ter_on = true; s->ter = *t; s->ter.early = a.early;
    return HSDDP_OK;
}

int hsddp_terrain_get_params(hsddp_sim_t* s, int* on, hsddp_terrain_t* t) {
    if (!s || !on || !t) return HSDDP_EINVAL;
    *on = s->ter_on ? 1 : 0; *t = s->ter;
    return HSDDP_OK;
}

int hsddp_terrain_get(hsddp_sim_t* s, int b0, int nb, hsddp_terrain_row_t* rows) {
    if (!sim_range_ok(s, b0, nb) || !rows || !s->last_ter) return HSDDP_EINVAL;
    return sim_fetch_rows(s, b0, nb, s->d_ter_rows, SIM_TER_ROW, [&](size_t i, const double* q) {
        rows[i].first_early = (int)q[0]; rows[i].n_early = (int)q[1]; rows[i].n_early_release = (int)q[2]; rows[i].n_held = (int)q[3]; rows[i].early_final = (int)q[4]; rows[i].pad = 0;
        rows[i].max_pen = q[5];
    });
}

int hsddp_friction_set(hsddp_sim_t* s, int on, const hsddp_friction_t* f, const double* mu, const int* mu_of) {
    if (!s) return HSDDP_EINVAL;
    if (!on) { s->fric_on = false; return HSDDP_OK; }      // later runs launch the kernels without friction; the buffers and the table are kept
    if (!f || !mu || f->n_mu < 1 || f->n_mu > 65536 || !std::isfinite(f->v_stick) || f->v_stick < 0.0) return HSDDP_EINVAL;
    for (int i = 0; i < f->n_mu; i++) {
        const double ms = mu[2 * i], mk = mu[2 * i + 1];
        if (!std::isfinite(ms) || !std::isfinite(mk) || mk < 0.0 || mk > ms) return HSDDP_EINVAL;
    }
    hsddp_handle* h = s->h;
    const size_t total = (size_t)h->batch * s->R;
    if (mu_of) for (size_t i = 0; i < total; i++) if (mu_of[i] < 0 || mu_of[i] >= f->n_mu) return HSDDP_EINVAL;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    if (!s->d_fric) SIM_CK(hipMalloc((void**)&s->d_fric, sizeof(WbsFricArgs)));      // (a failure: see SIM_CK - friction stays as it was)
    if (!s->d_fric_rows) SIM_CK(hipMalloc((void**)&s->d_fric_rows, total * SIM_FRIC_ROW * 8));
    if (!s->d_fric_of) SIM_CK(hipMalloc((void**)&s->d_fric_of, total * sizeof(int)));
    if (s->uni_keep && !s->d_fric_Sl) { SIM_CK(hipMalloc((void**)&s->d_fric_Sl, total * 4 * 8)); HIPCK(hipMemsetAsync(s->d_fric_Sl, 0, total * 4 * 8, h->stream)); }
    if (s->uni_keep && !s->d_fric_NF) { SIM_CK(hipMalloc((void**)&s->d_fric_NF, total * 4 * 8)); HIPCK(hipMemsetAsync(s->d_fric_NF, 0, total * 4 * 8, h->stream)); }
    if (!s->d_fric_H) { SIM_CK(hipMalloc((void**)&s->d_fric_H, 8)); HIPCK(hipMemsetAsync(s->d_fric_H, 0, 8, h->stream)); }
    if (!s->d_fric_tmap) { SIM_CK(hipMalloc((void**)&s->d_fric_tmap, total * sizeof(int))); HIPCK(hipMemsetAsync(s->d_fric_tmap, 0, total * sizeof(int), h->stream)); }
    if (!s->d_fric_trows) SIM_CK(hipMalloc((void**)&s->d_fric_trows, total * SIM_TER_ROW * 8));
    if (!s->d_fric_ter) {      // the flat map of runs with the terrain off: one cell of height 0, no early touchdown, E never carried (it stays empty)
        SIM_CK(hipMalloc((void**)&s->d_fric_ter, sizeof(WbsTerArgs)));
        WbsTerArgs t;
        t.H = s->d_fric_H; t.map_of = s->d_fric_tmap; t.nx = 1; t.ny = 1; t.n_maps = 1; t.early = 0;
        t.x0 = 0.0; t.y0 = 0.0; t.cx = 1.0; t.cy = 1.0; t.w_td = 0.0; t.rows = s->d_fric_trows; t.E = nullptr;
        HIPCK(hipMemcpyAsync(s->d_fric_ter, &t, sizeof(t), hipMemcpyHostToDevice, h->stream));
    }
    int rc = sim_ensure_records_and_trip_count(s);
    if (rc == HSDDP_OK) rc = sim_grow(h, s->d_fric_mu, s->fric_cap, (size_t)f->n_mu, 2);
    if (rc != HSDDP_OK) return rc;
    HIPCK(hipMemcpyAsync(s->d_fric_mu, mu, (size_t)f->n_mu * 2 * 8, hipMemcpyHostToDevice, h->stream));
    if (mu_of) HIPCK(hipMemcpyAsync(s->d_fric_of, mu_of, total * sizeof(int), hipMemcpyHostToDevice, h->stream));
    else HIPCK(hipMemsetAsync(s->d_fric_of, 0, total * sizeof(int), h->stream));
    WbsFricArgs a;
    a.mu = s->d_fric_mu; a.mu_of = s->d_fric_of; a.n_mu = f->n_mu; a.pad = 0; a.v_stick = f->v_stick; a.rows = s->d_fric_rows; a.Sl = s->d_fric_Sl; a.NF = s->d_fric_NF;      // (both or neither: a set call that failed between the two allocations returned above)
    HIPCK(hipMemcpyAsync(s->d_fric, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));      // mu and mu_of are the caller's: they may go once the call returns
    s->fric_on = true; s->fric.v_stick = f->v_stick; s->fric.n_mu = f->n_mu; s->fric.pad = 0;
    return HSDDP_OK;
}

int hsddp_friction_get_params(hsddp_sim_t* s, int* on, hsddp_friction_t* f) {
    if (!s || !on || !f) return HSDDP_EINVAL;
    *on = s->fric_on ? 1 : 0; *f = s->fric;
    return HSDDP_OK;
}

int hsddp_friction_get(hsddp_sim_t* s, int b0, int nb, hsddp_friction_row_t* rows) {
    if (!sim_range_ok(s, b0, nb) || !rows || !s->last_fric) return HSDDP_EINVAL;
    return sim_fetch_rows(s, b0, nb, s->d_fric_rows, SIM_FRIC_ROW, [&](size_t i, const double* q) {
        rows[i].first_slide = (int)q[0]; rows[i].n_onset = (int)q[1]; rows[i].n_slide = (int)q[2]; rows[i].n_restick = (int)q[3]; rows[i].slide_final = (int)q[4]; rows[i].pad = 0;
        rows[i].max_speed = q[5]; rows[i].distance = q[6];
    });
}

int hsddp_plant_set(hsddp_sim_t* s, int on, int n_plants, const double* P, const int* plant_of) {
    if (!s) return HSDDP_EINVAL;
    if (!on) { s->plant_on = false; return HSDDP_OK; }      // later runs launch the kernels without the plant; the buffers and the table are kept
    hsddp_handle* h = s->h;
    const size_t total = (size_t)h->batch * s->R;
    if (!plant_table_ok(n_plants, P, plant_of, total)) return HSDDP_EINVAL;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    std::vector<double> rows; std::vector<int> idx;
    plant_table_pack(n_plants, P, plant_of, total, rows, idx);
    if (!s->d_plant) SIM_CK(hipMalloc((void**)&s->d_plant, sizeof(WbsPlantArgs)));      // (a failure: see SIM_CK - the plant stays as it was)
    if (!s->d_plant_of) SIM_CK(hipMalloc((void**)&s->d_plant_of, total * sizeof(int)));
    int rc = sim_ensure_records_and_trip_count(s);
    if (rc == HSDDP_OK) rc = sim_grow(h, s->d_plant_P, s->plant_cap, (size_t)n_plants, SIM_PLANT_ROW);
    if (rc != HSDDP_OK) return rc;
    HIPCK(hipMemcpyAsync(s->d_plant_P, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCK(hipMemcpyAsync(s->d_plant_of, idx.data(), total * sizeof(int), hipMemcpyHostToDevice, h->stream));
    WbsPlantArgs a;
    a.P = s->d_plant_P; a.plant_of = s->d_plant_of; a.n_plants = n_plants; a.pad = 0;
    HIPCK(hipMemcpyAsync(s->d_plant, &a, sizeof(a), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));      // the sources are locals and the caller's: they may go once the call returns
    s->plant_on = true; s->n_plants = n_plants; s->plant_rows.swap(rows);
    return HSDDP_OK;
}

int hsddp_plant_get_params(hsddp_sim_t* s, int* on, int* n_plants) {
    if (!s || !on || !n_plants) return HSDDP_EINVAL;
    *on = s->plant_on ? 1 : 0; *n_plants = s->n_plants;
    return HSDDP_OK;
}

int hsddp_plant_get_table(hsddp_sim_t* s, int p0, int np, double* P) {
    if (!s || !P || np <= 0 || p0 < 0 || p0 > s->n_plants - np) return HSDDP_EINVAL;
    memcpy(P, s->plant_rows.data() + (size_t)p0 * SIM_PLANT_ROW, (size_t)np * SIM_PLANT_ROW * 8);
    return HSDDP_OK;
}

const double* hsddp_sim_device_final(hsddp_sim_t* s) { return s ? s->d_final : nullptr; }

int hsddp_sim_get_kernel_time_ms(hsddp_sim_t* s, float* ms) {
    if (!s || !ms || !s->timed) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(s->h->device));
    HIPCK(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return HSDDP_OK;
}


// ------------------------------------------------------------------------------------------------ MPC episodes (hsddp_episode.h)
}  // extern "C"
static_assert(sizeof(hsddp_episode_row_t) == sizeof(EpiRow), "the device row is hsddp_episode_row_t");
struct hsddp_episode {
    hsddp_handle* h = nullptr;
    hsddp_sim* sim = nullptr;                               // one sample per problem, n_exec steps, trajectories kept
    int n_exec = 0, max_ticks = 0, keep = 0, tick = 0, n_impacts = 0;
    bool started = false;                                   // hsddp_episode_reset has given the states
    int pending = -1;                                       // phase of the bound window whose reset map lies behind the tick's last step, else -1
    std::vector<int> map, map_new;                          // host copies of the step map: the bound one (source of the upload) / scratch of a rebind
    std::vector<EpiRow> row0;                               // [B] rows of a reset (source of the upload)
    double* d_state = nullptr; EpiRow* d_rows = nullptr;    // [B][36] ; [B]
    double *d_X = nullptr, *d_U = nullptr, *d_Y = nullptr;  // the log (keep): [B][max_ticks n_exec + 1][36], [B][max_ticks n_exec][12] twice
    // policy latency (hsddp_latency.h): everything below is allocated by hsddp_latency_set.  lat_on: what later ticks do; lat_valid: stash lat_cur holds
    // the rows the previous tick left; lat_ran: a tick has composed the effective rows; lat_dirty: the plan on the device is not that of (window, lat_D)
    bool lat_on = false, lat_valid = false, lat_ran = false, lat_dirty = false;
    int lat_D = 0, lat_cap = 0, lat_cur = 0;               // largest delay; rows a stash has room for; the stash the next tick READS
    std::vector<int> lat_delay, lat_long, lat_walk, lat_long_new, lat_walk_new;      // [B]; the plan of latency_plan.hpp on the device / scratch
    std::vector<LatPhase> lat_phases; std::vector<PhaseDev> lat_table;            // scratch of the plan; [n_exec] source of the table's upload
    int *d_lat_delay = nullptr, *d_lat_stale = nullptr, *d_lat_long = nullptr, *d_lat_walk = nullptr;      // [B] twice; [3][2 n_exec]; [3][n_exec]
    PhaseDev* d_lat_table = nullptr;                        // [n_exec] the descriptors the walk is sent to
    double *d_lat_X = nullptr, *d_lat_U = nullptr, *d_lat_K = nullptr, *d_lat_stash[2] = {nullptr, nullptr};      // episode.hpp: EpiLatArgs
};
static void episode_free(hsddp_episode* e) {
    if (!e) return;
    hipSetDevice(e->h->device);
    if (e->h->stream) hipStreamSynchronize(e->h->stream);
    if (e->sim) sim_free(e->sim);
    void* p[] = {e->d_state, e->d_rows, e->d_X, e->d_U, e->d_Y, e->d_lat_delay, e->d_lat_stale, e->d_lat_long, e->d_lat_walk, e->d_lat_table, e->d_lat_X, e->d_lat_U, e->d_lat_K,
                 e->d_lat_stash[0], e->d_lat_stash[1]};
    for (void* q : p) if (q) hipFree(q);
    delete e;
}
static bool episode_range_ok(const hsddp_episode* e, int b0, int nb) { return e && nb > 0 && b0 >= 0 && b0 <= e->h->batch - nb; }
// the plan of a tick with latency (latency_plan.hpp) for the handle's current window, into the scratch vectors; false: fewer than n_exec + lat_D leading whole-body knots
static bool episode_lat_plan(hsddp_episode* e) {
    const hsddp_handle* h = e->h;
    e->lat_phases.resize((size_t)h->nph);
    for (int i = 0; i < h->nph; i++) e->lat_phases[i] = LatPhase{h->ph[i].model == HSDDP_MODEL_WB ? 1 : 0, h->ph[i].h, h->ph[i].has_impact};
    int pend = -1;
    return lat_plan(e->lat_phases.data(), h->nph, e->n_exec, e->lat_D, e->lat_long_new.data(), e->lat_walk_new.data(), &pend);
}
// seed of tick t (hsddp_episode.h): the seed itself, then the raw outputs of SplitMix64(seed)
static unsigned long long episode_tick_seed(unsigned long long seed, int t) {
    if (t == 0) return seed;
    unsigned long long z = seed + (unsigned long long)t * WBS_MC_G;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

extern "C" {

int hsddp_episode_create(hsddp_handle_t* h, int n_exec, int max_ticks, int keep_log, hsddp_episode_t** out) {
    if (!h || !out || n_exec <= 0 || max_ticks <= 0 || h->f32) return HSDDP_EINVAL;
    const size_t B = h->batch, steps = (size_t)max_ticks * n_exec;
    if (steps >= ((size_t)1 << 31)) return HSDDP_ENOTSUP;      // global step indices are ints
    hsddp_sim* s = nullptr;
    int rc = hsddp_sim_create(h, 1, n_exec, 1, &s);
    if (rc != HSDDP_OK) return rc;
    hsddp_episode* e = new hsddp_episode();
    e->h = h; e->sim = s; e->n_exec = n_exec; e->max_ticks = max_ticks; e->keep = keep_log ? 1 : 0;
    e->map.assign(3 * (size_t)n_exec, 0); e->map_new.assign(3 * (size_t)n_exec, 0);
    sim_step_map(h, n_exec, e->map.data(), &e->pending);
    EpiRow r0{};
    r0.min_height = HUGE_VAL; r0.min_fz = HUGE_VAL; r0.min_cone = HUGE_VAL; r0.max_fz = -HUGE_VAL; r0.first_slip = -1; r0.end_step = -1;
    e->row0.assign(B, r0);
    SIM_CK_FREE(hipMalloc((void**)&e->d_state, B * 36 * 8), episode_free(e));
    SIM_CK_FREE(hipMalloc((void**)&e->d_rows, B * sizeof(EpiRow)), episode_free(e));
    if (e->keep) {
        SIM_CK_FREE(hipMalloc((void**)&e->d_X, B * (steps + 1) * 36 * 8), episode_free(e));
        SIM_CK_FREE(hipMalloc((void**)&e->d_U, B * steps * 12 * 8), episode_free(e));
        SIM_CK_FREE(hipMalloc((void**)&e->d_Y, B * steps * 12 * 8), episode_free(e));
        SIM_CK_FREE(hipMemset(e->d_X, 0, B * (steps + 1) * 36 * 8), episode_free(e));
        SIM_CK_FREE(hipMemset(e->d_U, 0, B * steps * 12 * 8), episode_free(e));
        SIM_CK_FREE(hipMemset(e->d_Y, 0, B * steps * 12 * 8), episode_free(e));
    }
    SIM_CK_FREE(hipMemset(e->d_state, 0, B * 36 * 8), episode_free(e));
    s->uni_keep = true; s->uni_hold = &e->d_rows[0].end_reason; s->uni_hold_stride = (int)(sizeof(EpiRow) / sizeof(int));      // (hsddp_contact.h: F lives across ticks, a frozen robot keeps its own)
    SIM_CK_FREE(hipMemcpy(e->d_rows, e->row0.data(), B * sizeof(EpiRow), hipMemcpyHostToDevice), episode_free(e));
    *out = e; return HSDDP_OK;
}

void hsddp_episode_destroy(hsddp_episode_t* e) { episode_free(e); }

int hsddp_episode_reset(hsddp_episode_t* e, const double* x0, int src_device) {
    if (!e || !x0) return HSDDP_EINVAL;
    hsddp_handle* h = e->h;
    const size_t B = h->batch, steps = (size_t)e->max_ticks * e->n_exec;
    HIPCK(hipSetDevice(h->device));
    HIPCK(hipMemcpyAsync(e->d_state, x0, B * 36 * 8, src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCK(hipMemcpyAsync(h->d_x0, e->d_state, B * 36 * 8, hipMemcpyDeviceToDevice, h->stream));      // what hsddp_set_initial_condition leaves
    HIPCK(hipMemcpyAsync(e->d_rows, e->row0.data(), B * sizeof(EpiRow), hipMemcpyHostToDevice, h->stream));
    if (e->keep) {
        HIPCK(hipMemsetAsync(e->d_X, 0, B * (steps + 1) * 36 * 8, h->stream)); HIPCK(hipMemsetAsync(e->d_U, 0, B * steps * 12 * 8, h->stream));
        HIPCK(hipMemsetAsync(e->d_Y, 0, B * steps * 12 * 8, h->stream));
    }
    if (e->sim->d_uni_F) HIPCK(hipMemsetAsync(e->sim->d_uni_F, 0, B * 4 * 8, h->stream));      // (hsddp_contact.h) every foot attached again
    if (e->sim->d_ter_E) HIPCK(hipMemsetAsync(e->sim->d_ter_E, 0, B * 4 * 8, h->stream));      // (hsddp_terrain.h) no swing foot held
    if (e->sim->d_fric_Sl) HIPCK(hipMemsetAsync(e->sim->d_fric_Sl, 0, B * 4 * 8, h->stream));      // (hsddp_friction.h) no foot sliding
    if (e->sim->d_fric_NF) HIPCK(hipMemsetAsync(e->sim->d_fric_NF, 0, B * 4 * 8, h->stream));
    if (e->d_lat_stale) HIPCK(hipMemsetAsync(e->d_lat_stale, 0, B * sizeof(int), h->stream));      // (hsddp_latency.h) nothing stale yet; the delays stay
    HIPCK(hipStreamSynchronize(h->stream));
    e->tick = 0; e->n_impacts = 0; e->started = true; e->lat_valid = false;
    return HSDDP_OK;
}

int hsddp_episode_advance(hsddp_episode_t* e, const hsddp_mc_dist_t* dist, const double* kick, int kick_device) {
    if (!e || !e->started || e->tick >= e->max_ticks) return HSDDP_EINVAL;
    hsddp_handle* h = e->h; hsddp_sim* s = e->sim;
    if (kick && !dist) return HSDDP_EINVAL;                       // (the step of the push is the disturbance's)
    if (dist && !mc_dist_ok(s, dist, kick)) return HSDDP_EINVAL;
    const bool moved = s->gen != h->window_gen;
    int pend = e->pending;
    if (moved && !sim_step_map(h, e->n_exec, e->map_new.data(), &pend)) return HSDDP_EINVAL;      // the window no longer leads with n_exec whole-body knots
    if (e->lat_on && !episode_lat_plan(e)) return HSDDP_EINVAL;      // (hsddp_latency.h) ... or not with the lat_D more the stash reads
    if (sim_unsupported(s)) return HSDDP_ENOTSUP;      // (hsddp_friction.h) before the rebind and the latency launch: the tick leaves nothing behind
    HIPCK(hipSetDevice(h->device));
    // rebind: the step map of the new window into the simulation object's buffer (the walk below synchronises the stream).  It stays in place if the
    // walk then fails with a device error - the map is that of the handle's current window either way; "nothing changed" is promised for HSDDP_EINVAL
    if (moved) {
        e->map.swap(e->map_new); e->pending = pend;
        HIPCK(hipMemcpyAsync(s->d_map, e->map.data(), e->map.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        s->gen = h->window_gen;
    }
    // policy latency (hsddp_latency.h): the plan of the bound window on the device, then ONE launch composes the rows this tick applies and stashes the
    // rows the next one may need - nothing between here and the end of the tick changes the handle's policy.  The walk is sent to the per-step table.
    if (e->lat_on) {
        const size_t B = (size_t)h->batch;
        const int n = e->n_exec, L = n + e->lat_D;
        if (moved || e->lat_dirty) {
            e->lat_long.swap(e->lat_long_new); e->lat_walk.swap(e->lat_walk_new);
            for (int q = 0; q < n; q++) {      // descriptor q: the step's phase with ONE knot, its policy at slice q of the effective rows
                PhaseDev c = h->ph[e->lat_long[q]];
                c.h = 1; c.Xbar = e->d_lat_X + (size_t)q * B * 72; c.Ubar = e->d_lat_U + (size_t)q * B * 12; c.K = e->d_lat_K + (size_t)q * B * 432;
                e->lat_table[q] = c;
            }
            HIPCK(hipMemcpyAsync(e->d_lat_long, e->lat_long.data(), 3 * (size_t)L * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCK(hipMemcpyAsync(e->d_lat_walk, e->lat_walk.data(), 3 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCK(hipMemcpyAsync(e->d_lat_table, e->lat_table.data(), (size_t)n * sizeof(PhaseDev), hipMemcpyHostToDevice, h->stream));
            e->lat_dirty = false;
        }
        EpiLatArgs la;
        la.n_exec = n; la.D = e->lat_D; la.B = h->batch; la.valid = e->lat_valid ? 1 : 0;
        la.map = e->d_lat_long; la.delay = e->d_lat_delay; la.n_stale = e->d_lat_stale; la.rows = e->d_rows;
        la.prev = e->d_lat_stash[e->lat_cur]; la.next = e->d_lat_stash[e->lat_cur ^ 1];
        la.Xe = e->d_lat_X; la.Ue = e->d_lat_U; la.Ke = e->d_lat_K;
        { Timed t(h, "k_episode_latency"); epi_latency_launch(h->stream, (unsigned)std::min<size_t>(B * L, LAT_MAX_WAVES), h->d_ph, la); }
        HIPCK(hipGetLastError());
        e->lat_valid = e->lat_D > 0; e->lat_cur ^= 1; e->lat_ran = true;
        s->walk_ph = e->d_lat_table; s->walk_map = e->d_lat_walk;
    } else e->lat_valid = false;      // a tick without latency leaves no stash
    int rc;
    if (!dist) rc = hsddp_sim_run(s, e->d_state, 1);
    else {
        hsddp_mc_dist_t d = *dist; d.seed = episode_tick_seed(dist->seed, e->tick);
        rc = hsddp_mc_run(s, e->d_state, 1, &d, kick, kick_device);
    }
    s->walk_ph = nullptr; s->walk_map = nullptr;
    if (rc != HSDDP_OK) return rc;
    EpiCommitArgs a;
    a.n_exec = e->n_exec; a.tick = e->tick; a.max_ticks = e->max_ticks; a.handoff = e->pending < 0 ? 1 : 0;
    a.map = s->d_map; a.simX = s->d_X; a.simU = s->d_U; a.simY = s->last_grf ? s->d_Y : nullptr;
    a.fin = s->d_final; a.sim_rows = s->d_rows; a.extra = s->last_mc == 1 ? s->d_extra : nullptr; a.grf_rows = s->last_grf ? s->d_grf_rows : nullptr;
    a.st = h->d_st; a.rows = e->d_rows; a.state = e->d_state; a.x0 = h->d_x0;
    a.logX = e->d_X; a.logU = e->d_U; a.logY = e->d_Y;
    // (both kernels are timed into the handle's kernel table, hsddp_get_kernel_times, like the solver's; the walk's time is the simulation object's)
    { Timed t(h, "k_episode_commit"); hipLaunchKernelGGL(k_episode_commit, dim3((unsigned)h->batch), dim3(64), 0, h->stream, h->d_ph, a); }
    if (e->pending >= 0) {      // the tick ended on a touchdown: the reset map the moved window no longer holds
        Timed t(h, s->plant_on ? "k_episode_impact_plant" : "k_episode_impact");
        if (s->plant_on)      // (hsddp_plant.h) the same map with each robot's own inertias
            wbs_plant_impact_launch(h->stream, (unsigned)((h->batch + 15) / 16), h->d_ph, h->md, e->pending, h->batch, &e->d_rows[0].end_reason, (int)(sizeof(EpiRow) / sizeof(int)), e->d_state, h->d_x0, s->d_plant);
        else
            hipLaunchKernelGGL(k_episode_impact, dim3((unsigned)((h->batch + 15) / 16)), dim3(64), 0, h->stream, h->d_ph, h->md, e->pending, h->batch, (const EpiRow*)e->d_rows, e->d_state, h->d_x0);
        e->n_impacts++;
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(h->stream));
    drain_events(h);
    e->tick++;
    return HSDDP_OK;
}

int hsddp_episode_get_rows(hsddp_episode_t* e, int b0, int nb, hsddp_episode_row_t* rows, double* x_now) {
    if (!episode_range_ok(e, b0, nb) || !rows) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(e->h->device));
    HIPCK(hipMemcpy(rows, e->d_rows + b0, (size_t)nb * sizeof(EpiRow), hipMemcpyDeviceToHost));
    if (x_now) HIPCK(hipMemcpy(x_now, e->d_state + (size_t)b0 * 36, (size_t)nb * 36 * 8, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_episode_get_log(hsddp_episode_t* e, int b0, int nb, double* X, double* U, double* Y) {
    if (!episode_range_ok(e, b0, nb) || !e->keep) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(e->h->device));
    const size_t steps = (size_t)e->max_ticks * e->n_exec, sx = (steps + 1) * 36, su = steps * 12;
    if (X) HIPCK(hipMemcpy(X, e->d_X + (size_t)b0 * sx, (size_t)nb * sx * 8, hipMemcpyDeviceToHost));
    if (U) HIPCK(hipMemcpy(U, e->d_U + (size_t)b0 * su, (size_t)nb * su * 8, hipMemcpyDeviceToHost));
    if (Y) HIPCK(hipMemcpy(Y, e->d_Y + (size_t)b0 * su, (size_t)nb * su * 8, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_latency_set(hsddp_episode_t* e, int on, const int* delay_of, int delay) {
    if (!e) return HSDDP_EINVAL;
    if (!on) { e->lat_on = false; e->lat_valid = false; return HSDDP_OK; }      // later ticks launch what they launched without it; the buffers and the delays are kept
    hsddp_handle* h = e->h;
    const size_t B = (size_t)h->batch, n = (size_t)e->n_exec;
    int D = 0;
    for (size_t b = 0; b < B; b++) {
        const int d = delay_of ? delay_of[b] : delay;
        if (d < 0 || d > e->n_exec) return HSDDP_EINVAL;
        D = std::max(D, d);
    }
    HIPCK(hipSetDevice(h->device));
    if (!e->d_lat_delay) SIM_CK(hipMalloc((void**)&e->d_lat_delay, B * sizeof(int)));      // (a failure: see SIM_CK - latency stays as it was)
    if (!e->d_lat_stale) { SIM_CK(hipMalloc((void**)&e->d_lat_stale, B * sizeof(int))); HIPCK(hipMemsetAsync(e->d_lat_stale, 0, B * sizeof(int), h->stream)); }
    if (!e->d_lat_long) SIM_CK(hipMalloc((void**)&e->d_lat_long, 3 * 2 * n * sizeof(int)));      // (room for the largest D there is, n_exec)
    if (!e->d_lat_walk) SIM_CK(hipMalloc((void**)&e->d_lat_walk, 3 * n * sizeof(int)));
    if (!e->d_lat_table) SIM_CK(hipMalloc((void**)&e->d_lat_table, n * sizeof(PhaseDev)));
    if (!e->d_lat_X) SIM_CK(hipMalloc((void**)&e->d_lat_X, n * B * 72 * 8));
    if (!e->d_lat_U) SIM_CK(hipMalloc((void**)&e->d_lat_U, n * B * 12 * 8));
    if (!e->d_lat_K) SIM_CK(hipMalloc((void**)&e->d_lat_K, n * B * 432 * 8));
    if (D > e->lat_cap) {      // the new pair first, so that a failure leaves the old one in place
        double* nb[2] = {nullptr, nullptr};
        SIM_CK(hipMalloc((void**)&nb[0], B * (size_t)D * LAT_ROW * 8));
        SIM_CK_FREE(hipMalloc((void**)&nb[1], B * (size_t)D * LAT_ROW * 8), hipFree(nb[0]));
        HIPCK(hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; i++) { if (e->d_lat_stash[i]) hipFree(e->d_lat_stash[i]); e->d_lat_stash[i] = nb[i]; }
        e->lat_cap = D;
    }
    e->lat_delay.resize(B);
    for (size_t b = 0; b < B; b++) e->lat_delay[b] = delay_of ? delay_of[b] : delay;
    e->lat_long.assign(3 * 2 * n, 0); e->lat_long_new.assign(3 * 2 * n, 0); e->lat_walk.assign(3 * n, 0); e->lat_walk_new.assign(3 * n, 0); e->lat_table.resize(n);
    HIPCK(hipMemcpyAsync(e->d_lat_delay, e->lat_delay.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    e->lat_on = true; e->lat_D = D; e->lat_valid = false; e->lat_dirty = true;      // (the stash rows are laid out for the old D: the next tick runs fresh)
    return HSDDP_OK;
}

int hsddp_latency_get(hsddp_episode_t* e, int b0, int nb, hsddp_latency_row_t* rows) {
    if (!episode_range_ok(e, b0, nb) || !rows || !e->d_lat_stale) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(e->h->device));
    std::vector<int> st((size_t)nb);
    HIPCK(hipMemcpy(st.data(), e->d_lat_stale + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < nb; i++) { rows[i].delay = e->lat_delay[(size_t)b0 + i]; rows[i].n_stale = st[i]; }
    return HSDDP_OK;
}

int hsddp_latency_get_policy(hsddp_episode_t* e, int b0, int nb, double* Xe, double* Ue, double* Ke) {
    if (!episode_range_ok(e, b0, nb) || !e->lat_ran) return HSDDP_EINVAL;
    HIPCK(hipSetDevice(e->h->device));
    const size_t B = (size_t)e->h->batch, n = (size_t)e->n_exec;
    std::vector<double> tmp((size_t)nb * 432);
    const double* src[3] = {e->d_lat_X, e->d_lat_U, e->d_lat_K}; double* dst[3] = {Xe, Ue, Ke}; const size_t w[3] = {72, 12, 432};
    for (int a = 0; a < 3; a++) {      // the device keeps the rows step-major (episode.hpp), the caller gets them problem-major
        if (!dst[a]) continue;
        for (size_t q = 0; q < n; q++) {
            HIPCK(hipMemcpy(tmp.data(), src[a] + (q * B + (size_t)b0) * w[a], (size_t)nb * w[a] * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < (size_t)nb; i++) memcpy(dst[a] + (i * n + q) * w[a], tmp.data() + i * w[a], w[a] * 8);
        }
    }
    return HSDDP_OK;
}

const double* hsddp_episode_device_state(hsddp_episode_t* e) { return e ? e->d_state : nullptr; }
hsddp_sim_t* hsddp_episode_sim(hsddp_episode_t* e) { return e ? e->sim : nullptr; }

int hsddp_episode_status(hsddp_episode_t* e, int* tick, int* n_alive, int* n_impacts) {
    if (!e) return HSDDP_EINVAL;
    if (n_alive) {
        HIPCK(hipSetDevice(e->h->device));
        std::vector<EpiRow> r((size_t)e->h->batch);
        HIPCK(hipMemcpy(r.data(), e->d_rows, r.size() * sizeof(EpiRow), hipMemcpyDeviceToHost));
        int n = 0; for (const EpiRow& q : r) n += q.end_reason == 0 ? 1 : 0;
        *n_alive = n;
    }
    if (tick) *tick = e->tick;
    if (n_impacts) *n_impacts = e->n_impacts;
    return HSDDP_OK;
}

}  // extern "C"
