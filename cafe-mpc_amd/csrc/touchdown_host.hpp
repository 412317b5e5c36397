// Host side of include/hsddp_touchdown.h.  Part of hsddp_hip.hip's translation unit, host pass only (behind sim_host.hpp: the episode call reads the
// terrain its simulation object holds).
//
// Storage: ONE table per handle, d_tdh [nph_cap][batch][4] doubles (phase-major, by leg), allocated by the first call that needs it and never again -
// nph_cap and batch are fixed at hsddp_create - and handed to the _tdh rollout kernels as an argument.  td_own[phase] marks the phases with heights of
// their own, td_n counts them.  Invariant while td_n > 0: the rows of every other phase hold that phase's ground_height, so the _tdh kernels read the
// table for every whole-body terminal knot and a phase without heights of its own still computes foot_z - ground_height.  td_n == 0: the table is
// not read at all, roll_pick (roll_pick.hpp) names the kernels that were always launched.
#pragma once
#include "hsddp_touchdown.h"
#include "touchdown.hpp"

static int ws_tdh_ready(hsddp_handle* h);      // weights_host.hpp

static hs::TdHandleInfo td_info(const hsddp_handle* h) { return hs::TdHandleInfo{h->nph, h->batch, h->f32 ? 1 : 0}; }
static std::vector<hs::TdPhaseInfo> td_phases(const hsddp_handle* h) {
    std::vector<hs::TdPhaseInfo> v(h->nph);
    for (int i = 0; i < h->nph; i++) v[i] = hs::TdPhaseInfo{h->ph[i].model, h->ph[i].nt};
    return v;
}
static int td_ensure(hsddp_handle* h) {
    if ((int)h->td_own.size() != h->nph) { h->td_own.assign(h->nph, 0); h->td_n = 0; }
    if (h->d_tdh) return HSDDP_OK;
    HIPCK(hipMalloc((void**)&h->d_tdh, (size_t)h->nph_cap * h->batch * 4 * sizeof(double)));
    return HSDDP_OK;
}
// rows of phases [p0, p1) <- their descriptor's ground_height
static int td_fill(hsddp_handle* h, int p0, int p1) {
    const size_t row = (size_t)h->batch * 4;
    h->td_stage.resize((size_t)(p1 - p0) * row);
    for (int pi = p0; pi < p1; pi++) std::fill(h->td_stage.begin() + (size_t)(pi - p0) * row, h->td_stage.begin() + (size_t)(pi - p0 + 1) * row, h->ph[pi].ground_height);
    HIPCK(hipMemcpyAsync(h->d_tdh + (size_t)p0 * row, h->td_stage.data(), h->td_stage.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));      // (td_stage is the source)
    return HSDDP_OK;
}
// one k_td_terrain launch over the window from a grid in device memory; every whole-body phase with a touchdown constraint then has heights of its own
static int td_from_grid(hsddp_handle* h, const hs::TdGrid& g) {
    { const int rc = td_ensure(h); if (rc) return rc; }
    int n = 0; for (int i = 0; i < h->nph; i++) if (h->ph[i].model == HSDDP_MODEL_WB && h->ph[i].nt > 0) n++;
    if (n == 0) return HSDDP_OK;
    {
        Timed t(h, "k_td_terrain");
        launch_k_td_terrain(h->stream, h->d_ph, h->nph, h->batch, g, h->d_tdh);
    }
    HIPCK(hipGetLastError());
    for (int i = 0; i < h->nph; i++) h->td_own[i] = (h->ph[i].model == HSDDP_MODEL_WB && h->ph[i].nt > 0) ? 1 : 0;
    h->td_n = n; h->td_shared_gen = -1;
    return HSDDP_OK;
}

extern "C" {

int hsddp_touchdown_set(hsddp_handle_t* h, int phase, int b0, int nb, const double* heights, int src_device) {
    if (!h) return HSDDP_EINVAL;
    { const auto ph = td_phases(h); const int rc = hs::td_check_set(td_info(h), ph.data(), phase, b0, nb, heights, src_device); if (rc) return rc; }
    HIPCK(hipSetDevice(h->device));
    { const int rc = td_ensure(h); if (rc) return rc; }
    if (h->td_n == 0) { const int rc = td_fill(h, 0, h->nph); if (rc) return rc; }      // (later first calls find their rows filled: the invariant above)
    double* dst = h->d_tdh + ((size_t)phase * h->batch + b0) * 4;
    HIPCK(hipMemcpyAsync(dst, heights, (size_t)nb * 4 * sizeof(double), src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));      // the new heights are in place on return; a host source may be reused
    if (!h->td_own[phase]) { h->td_own[phase] = 1; h->td_n++; }
    h->td_shared_gen = -1;      // (weights_host.hpp: the table no longer holds the shared value in every row)
    return HSDDP_OK;
}

int hsddp_touchdown_get(hsddp_handle_t* h, int phase, int b0, int nb, double* heights, double* values) {
    if (!h) return HSDDP_EINVAL;
    { const auto ph = td_phases(h); const int rc = hs::td_check_range(td_info(h), ph.data(), phase, b0, nb); if (rc) return rc; }
    HIPCK(hipSetDevice(h->device));
    HIPCK(hipStreamSynchronize(h->stream));
    const PhaseDev& P = h->ph[phase];
    if (heights) {
        if ((int)h->td_own.size() == h->nph && h->td_own[phase]) HIPCK(hipMemcpy(heights, h->d_tdh + ((size_t)phase * h->batch + b0) * 4, (size_t)nb * 4 * sizeof(double), hipMemcpyDeviceToHost));
        else std::fill(heights, heights + (size_t)nb * 4, P.ground_height);
    }
    if (values) {
        std::vector<double> th((size_t)nb * P.nt);
        HIPCK(hipMemcpy(th.data(), P.th + (size_t)b0 * P.nt, th.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int b = 0; b < nb; b++) {
            int i = 0;
            for (int f = 0; f < 4; f++) values[(size_t)b * 4 + f] = (P.td[f] && i < P.nt) ? th[(size_t)b * P.nt + i++] : std::nan("");
        }
    }
    return HSDDP_OK;
}

int hsddp_touchdown_clear(hsddp_handle_t* h, int phase) {
    if (!h || phase < -1 || phase >= h->nph) return HSDDP_EINVAL;
    if ((int)h->td_own.size() != h->nph || h->td_n == 0) return HSDDP_OK;
    if (phase >= 0 && !h->td_own[phase]) return HSDDP_OK;
    HIPCK(hipSetDevice(h->device));
    if (phase < 0 || h->td_n == 1) { h->td_own.assign(h->nph, 0); h->td_n = 0; return ws_tdh_ready(h); }      // (scales in use: their terminal programs go on reading the table)
    { const int rc = td_fill(h, phase, phase + 1); if (rc) return rc; }      // other phases keep theirs: this one reads the shared value from the table
    h->td_own[phase] = 0; h->td_n--;
    return HSDDP_OK;
}

int hsddp_touchdown_from_terrain(hsddp_handle_t* h, const hsddp_terrain_t* t, const double* H, const int* map_of, double z_ground, int src_device) {
    if (!h || !t) return HSDDP_EINVAL;
    { const int rc = hs::td_check_terrain(td_info(h), t->nx, t->ny, t->n_maps, t->x0, t->y0, t->cx, t->cy, z_ground, H, map_of, src_device); if (rc) return rc; }
    HIPCK(hipSetDevice(h->device));
    hs::TdGrid g{H, map_of, 1, t->nx, t->ny, t->n_maps, t->x0, t->y0, t->cx, t->cy, z_ground};
    if (!src_device) {      // staged in handle-owned buffers that only grow
        const size_t cells = (size_t)t->n_maps * t->nx * t->ny;
        if (cells > h->td_H_cap) {
            HIPCK(hipStreamSynchronize(h->stream));
            if (h->d_td_H) HIPCK(hipFree(h->d_td_H)); h->d_td_H = nullptr; h->td_H_cap = 0;
            HIPCK(hipMalloc((void**)&h->d_td_H, cells * sizeof(double))); h->td_H_cap = cells;
        }
        if (map_of && !h->d_td_map) HIPCK(hipMalloc((void**)&h->d_td_map, (size_t)h->batch * sizeof(int)));
        HIPCK(hipMemcpyAsync(h->d_td_H, H, cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (map_of) HIPCK(hipMemcpyAsync(h->d_td_map, map_of, (size_t)h->batch * sizeof(int), hipMemcpyHostToDevice, h->stream));
        g.H = h->d_td_H; g.map_of = map_of ? h->d_td_map : nullptr;
    }
    const int rc = td_from_grid(h, g);
    HIPCK(hipStreamSynchronize(h->stream));      // H and map_of are the caller's: they may go once the call returns
    drain_events(h);                             // (k_td_terrain's time is in hsddp_get_kernel_times from here on)
    return rc;
}

int hsddp_episode_plan_terrain(hsddp_episode_t* e) {
    if (!e || !e->sim || !e->sim->ter_on || !e->sim->d_ter_H || !e->sim->d_ter_map) return HSDDP_EINVAL;
    hsddp_handle* h = e->h; const hsddp_sim* s = e->sim;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    const hs::TdGrid g{s->d_ter_H, s->d_ter_map, s->R, s->ter.nx, s->ter.ny, s->ter.n_maps, s->ter.x0, s->ter.y0, s->ter.cx, s->ter.cy, s->uni_z_ground};
    return td_from_grid(h, g);      // (stream order: the solve that follows is launched on the same stream)
}

}  // extern "C"
