// Host side of include/hsddp_limits.h.  Part of hsddp_hip.hip's translation unit, host pass only (behind weights_host.hpp: the kernels with limits
// have the scales and the touchdown heights compiled in and read those headers' tables).
//
// Storage: ONE device block per handle, d_lim, allocated by the first hsddp_limits_set / hsddp_episode_plan_friction and never again (batch and
// nph_cap are fixed at hsddp_create):
//     user [batch][12]  |  staging of a host source [batch][12]  |  resolved [nph_cap][batch][12]  |  descriptor rows [nph_cap][12]  |  ones [batch][84]
// lim_on: the table is in use (hsddp_limits_clear only drops the flag; the next set starts from NaN again).  Whether a launch reads the
// resolved table is roll_pick's rule (roll_pick.hpp: in use, fp64, a whole-body phase and no kinodynamic one in the window); otherwise exactly the
// kernels of before are launched.  `ones` is the scale table the rule names for the _lim kernels while hsddp_weights.h has none set; ws_on and d_ws are not touched.
#pragma once
#include "hsddp_limits.h"
#include "limits.hpp"

static_assert(hs::LIM_OK == HSDDP_OK && hs::LIM_EINVAL == HSDDP_EINVAL && hs::LIM_ENOTSUP == HSDDP_ENOTSUP, "limits.hpp repeats the return codes of hsddp.h");
static_assert(hs::LMP_ROW == hs::LIM_ROW && hs::LMP_ROW == HSDDP_LIMITS_ROW && hs::LMP_TORQUE == hs::LIM_TORQUE && hs::LMP_JLB == hs::LIM_JLB && hs::LMP_JUB == hs::LIM_JUB &&
              hs::LMP_HMIN == hs::LIM_HMIN && hs::LMP_MU == hs::LIM_MU && hs::LMP_JSLB == hs::LIM_JSLB && hs::LMP_JSUB == hs::LIM_JSUB, "one row layout");

static hs::LimHandleInfo lim_info(const hsddp_handle* h) { return hs::LimHandleInfo{h->batch, h->nph, h->f32 ? 1 : 0}; }
// the limits of a phase descriptor as a row
static void lim_desc_row(const PhaseDev& P, double* r) {
    r[hs::LMP_TORQUE] = P.torque_limit;
    for (int j = 0; j < 3; j++) { r[hs::LMP_JLB + j] = P.joint_lb[j]; r[hs::LMP_JUB + j] = P.joint_ub[j]; }
    r[hs::LMP_HMIN] = P.h_min; r[hs::LMP_MU] = P.mu; r[hs::LMP_JSLB] = P.jspeed_lb; r[hs::LMP_JSUB] = P.jspeed_ub; r[hs::LMP_PAD] = 0.0;
}
static int lim_ensure(hsddp_handle* h) {
    if (h->d_lim) return HSDDP_OK;
    const size_t n = lim_off_ones(h) + (size_t)h->batch * hs::WS_ROW;
    HIPCK(hipMalloc((void**)&h->d_lim, n * sizeof(double)));
    std::vector<double> ones((size_t)h->batch * hs::WS_ROW, 1.0);
    HIPCK(hipMemcpy(h->d_lim + lim_off_ones(h), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    h->lim_desc.assign((size_t)h->nph_cap * hs::LMP_ROW, 0.0);
    return HSDDP_OK;
}
// the current window's descriptor rows -> device (the source is the handle's: in place once the stream has passed the copy)
static int lim_upload_desc(hsddp_handle* h) {
    for (int i = 0; i < h->nph; i++) lim_desc_row(h->ph[i], h->lim_desc.data() + (size_t)i * hs::LMP_ROW);
    HIPCK(hipMemcpyAsync(h->d_lim + lim_off_desc(h), h->lim_desc.data(), (size_t)h->nph * hs::LMP_ROW * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return HSDDP_OK;
}
static hs::LimPack lim_pack_args(hsddp_handle* h, const double* src, int b0, int nb, int p0, int np, int mode) {
    return hs::LimPack{h->d_lim, h->d_lim + lim_off_res(h), src, h->d_lim + lim_off_desc(h), h->batch, h->nph, b0, nb, p0, np, mode};
}
// hsddp_reconfigure while a table is set: the user rows against the new window's descriptors, one launch
static int lim_repack(hsddp_handle* h) {
    if (!h->lim_on || h->f32) return HSDDP_OK;
    { const int rc = lim_upload_desc(h); if (rc) return rc; }
    {
        Timed t(h, "k_pack_limits");
        launch_k_pack_limits(h->stream, lim_pack_args(h, nullptr, 0, 0, 0, h->batch, hs::LIM_PACK_RESOLVE));
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(h->stream));      // (lim_desc is the copy's source and the next reconfigure rewrites it)
    return HSDDP_OK;
}
// first use: the table with every entry NaN, resolved against the window (hsddp_episode_plan_friction on a handle without limits)
static int lim_start(hsddp_handle* h, const double* src, int b0, int nb) {
    { const int rc = lim_ensure(h); if (rc) return rc; }
    { const int rc = lim_upload_desc(h); if (rc) return rc; }
    const bool first = !h->lim_on;
    {
        Timed t(h, "k_pack_limits");
        launch_k_pack_limits(h->stream, lim_pack_args(h, src, b0, nb, first ? 0 : b0, first ? h->batch : nb, first ? hs::LIM_PACK_FIRST : hs::LIM_PACK_RANGE));
    }
    HIPCK(hipGetLastError());
    h->lim_on = true;
    return HSDDP_OK;
}

extern "C" {

int hsddp_limits_set(hsddp_handle_t* h, int b0, int nb, const double* rows, int src_device) {
    if (!h) return HSDDP_EINVAL;
    { const int rc = hs::lim_check_set(lim_info(h), b0, nb, rows, src_device); if (rc) return rc; }
    HIPCK(hipSetDevice(h->device));
    { const int rc = lim_ensure(h); if (rc) return rc; }
    const double* src = rows;
    if (!src_device) {
        double* stage = h->d_lim + (size_t)h->batch * hs::LMP_ROW;
        HIPCK(hipMemcpyAsync(stage, rows, (size_t)nb * hs::LMP_ROW * sizeof(double), hipMemcpyHostToDevice, h->stream));
        src = stage;
    }
    { const int rc = lim_start(h, src, b0, nb); if (rc) return rc; }
    HIPCK(hipStreamSynchronize(h->stream));      // the rows are in place on return; the caller's source may go
    drain_events(h);
    return ws_tdh_ready(h);
}

int hsddp_limits_get(hsddp_handle_t* h, int phase, int b0, int nb, double* rows) {
    if (!h || !rows) return HSDDP_EINVAL;
    { const int rc = hs::lim_check_get(lim_info(h), phase, b0, nb); if (rc) return rc; }
    if (!h->lim_on) {
        for (int b = 0; b < nb; b++) lim_desc_row(h->ph[phase], rows + (size_t)b * hs::LMP_ROW);
        return HSDDP_OK;
    }
    HIPCK(hipSetDevice(h->device));
    HIPCK(hipStreamSynchronize(h->stream));
    HIPCK(hipMemcpy(rows, h->d_lim + lim_off_res(h) + ((size_t)phase * h->batch + b0) * hs::LMP_ROW, (size_t)nb * hs::LMP_ROW * sizeof(double), hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_limits_clear(hsddp_handle_t* h) {
    if (!h) return HSDDP_EINVAL;
    if (h->f32) return HSDDP_ENOTSUP;
    h->lim_on = false;
    return HSDDP_OK;
}

int hsddp_episode_plan_friction(hsddp_episode_t* e, double kappa) {
    if (!e || !e->sim || !e->sim->fric_on || !e->sim->d_fric_mu || !e->sim->d_fric_of) return HSDDP_EINVAL;
    if (hs::lim_check_kappa(kappa)) return HSDDP_EINVAL;
    hsddp_handle* h = e->h; const hsddp_sim* s = e->sim;
    if (h->f32) return HSDDP_ENOTSUP;
    HIPCK(hipSetDevice(h->device));
    if (!h->lim_on) {      // no table yet: every entry NaN, resolved against the window; the launch below then writes the mu column
        { const int rc = lim_ensure(h); if (rc) return rc; }
        { const int rc = lim_start(h, nullptr, 0, 0); if (rc) return rc; }
        { const int rc = ws_tdh_ready(h); if (rc) return rc; }
        HIPCK(hipStreamSynchronize(h->stream));      // (first call only: lim_desc is the source of the descriptor rows' copy)
    }
    {
        Timed t(h, "k_lim_mu");
        launch_k_lim_mu(h->stream, hs::LimMu{h->d_lim, h->d_lim + lim_off_res(h), s->d_fric_mu, s->d_fric_of, s->R, h->batch, h->nph, kappa});
    }
    HIPCK(hipGetLastError());
    return HSDDP_OK;      // (stream order: the solve that follows is launched on the same stream)
}

}  // extern "C"
