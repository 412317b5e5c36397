// Host side of include/hsddp_weights.h.  Part of hsddp_hip.hip's translation unit, host pass only (behind touchdown_host.hpp: the scaled terminal
// programs read that header's table).
//
// Storage: ONE device block per handle, d_ws = [2][batch][84] doubles, allocated by the first hsddp_weights_set and never again: the first half is
// the table the _pw kernels read, the second half stages a host source for k_pack_weights.  ws_on: the table is in use (hsddp_weights_clear only
// drops the flag; the next set starts from 1.0 again).  Whether a launch reads it is roll_pick's rule (roll_pick.hpp: in use, fp64, a
// whole-body phase and no kinodynamic one in the window); otherwise exactly the kernels of before are launched, with no table.
//
// Touchdown heights: k_rollout_pw and k_rollout_quad_term_pw have them compiled in and read d_tdh for every whole-body terminal knot.  While no
// phase has heights of its own (td_n == 0) ws_tdh_ready keeps that table filled with every phase's ground_height for the CURRENT window
// (td_shared_gen == window_gen); touchdown_host.hpp drops the mark when it writes heights of a phase's own.
#pragma once
#include "hsddp_weights.h"
#include "weights.hpp"

static_assert(hs::WS_OK == HSDDP_OK && hs::WS_EINVAL == HSDDP_EINVAL && hs::WS_ENOTSUP == HSDDP_ENOTSUP, "weights.hpp repeats the return codes of hsddp.h");
static_assert(hs::WSP_ROW == hs::WS_ROW && hs::WSP_R == hs::WS_R && hs::WSP_QF == hs::WS_QF && hs::WSP_ROW == HSDDP_WEIGHTS_ROW, "one row layout");

static int ws_tdh_ready(hsddp_handle* h) {
    if ((!h->ws_on && !h->lim_on) || h->f32) return HSDDP_OK;      // (the kernels with limits, hsddp_limits.h, have the heights compiled in as well)
    if ((int)h->td_own.size() == h->nph && h->td_n > 0) return HSDDP_OK;      // touchdown_host.hpp's invariant holds the other phases' rows
    if (h->d_tdh && h->td_shared_gen == h->window_gen) return HSDDP_OK;
    { const int rc = td_ensure(h); if (rc) return rc; }
    { const int rc = td_fill(h, 0, h->nph); if (rc) return rc; }
    h->td_shared_gen = h->window_gen;
    return HSDDP_OK;
}

extern "C" {

int hsddp_weights_set(hsddp_handle_t* h, int b0, int nb, const double* scales, int src_device) {
    if (!h) return HSDDP_EINVAL;
    { const int rc = hs::ws_check_set(hs::WsHandleInfo{h->batch, h->f32 ? 1 : 0}, b0, nb, scales, src_device); if (rc) return rc; }
    HIPCK(hipSetDevice(h->device));
    const size_t tab = (size_t)h->batch * hs::WSP_ROW;
    if (!h->d_ws) HIPCK(hipMalloc((void**)&h->d_ws, 2 * tab * sizeof(double)));
    const double* src = scales;
    if (!src_device) {
        double* stage = h->d_ws + tab;
        HIPCK(hipMemcpyAsync(stage, scales, (size_t)nb * hs::WSP_ROW * sizeof(double), hipMemcpyHostToDevice, h->stream));
        src = stage;
    }
    const bool first = !h->ws_on;
    const hs::WsPack W{h->d_ws, src, b0, nb, first ? 0 : b0, first ? h->batch : nb};
    {
        Timed t(h, "k_pack_weights");
        launch_k_pack_weights(h->stream, W);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(h->stream));      // the rows are in place on return; the caller's source may go
    drain_events(h);
    h->ws_on = true;
    return ws_tdh_ready(h);
}

int hsddp_weights_get(hsddp_handle_t* h, int b0, int nb, double* scales) {
    if (!h || !scales) return HSDDP_EINVAL;
    { const int rc = hs::ws_check_range(hs::WsHandleInfo{h->batch, h->f32 ? 1 : 0}, b0, nb); if (rc) return rc; }
    if (!h->ws_on) { std::fill(scales, scales + (size_t)nb * hs::WSP_ROW, 1.0); return HSDDP_OK; }
    HIPCK(hipSetDevice(h->device));
    HIPCK(hipStreamSynchronize(h->stream));
    HIPCK(hipMemcpy(scales, h->d_ws + (size_t)b0 * hs::WSP_ROW, (size_t)nb * hs::WSP_ROW * sizeof(double), hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

int hsddp_weights_clear(hsddp_handle_t* h) {
    if (!h) return HSDDP_EINVAL;
    if (h->f32) return HSDDP_ENOTSUP;
    h->ws_on = false;
    return HSDDP_OK;
}

}  // extern "C"
