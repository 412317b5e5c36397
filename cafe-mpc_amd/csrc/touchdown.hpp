// Per-problem touchdown heights (include/hsddp_touchdown.h): what needs no HIP - the argument rules of the C-ABI and the terrain lookup behind
// k_td_terrain.  Compiled for the device by hsddp_tdh.hip and for the host by the library and by the tests (TOUCHDOWN_HOST_ONLY: no HIP headers, the
// kernel's loop as td_terrain_host).
//
//   td_check_set / td_check_range / td_check_terrain   pure functions of the call's arguments and of what the handle knows about the phase; the
//                 library calls them before it touches anything, tests/cpp/touchdown_table.cpp walks them on their own.
//   td_terrain_height   the height one lane of k_td_terrain stores: z_ground + H[m][iy][ix] at the phase's TERMINAL reference foothold of leg l, the
//                 lookup of hsddp_terrain.h (wbs_ter_height_lane, wb_sim.hpp): the cell index is clamped as a double - fmax / fmin drop a NaN, which
//                 therefore reads cell 0 - before it becomes an integer.
#pragma once
#include <cmath>
#include <cstddef>

#ifdef TOUCHDOWN_HOST_ONLY
#define TD_HD inline
#else
#define TD_HD __host__ __device__ inline
#endif

namespace hs {

// return codes of include/hsddp.h (HSDDP_OK, HSDDP_EINVAL, HSDDP_ENOTSUP), repeated so that this header stands alone
enum { TD_OK = 0, TD_EINVAL = -1, TD_ENOTSUP = -4 };
enum { TD_MODEL_WB = 0 };      // HSDDP_MODEL_WB

// what the rules need to know about a handle and one of its phases
struct TdPhaseInfo { int model, nt; };
struct TdHandleInfo { int nph, batch, f32; };

// phase / range of hsddp_touchdown_set and hsddp_touchdown_get
inline int td_check_range(const TdHandleInfo& h, const TdPhaseInfo* ph, int phase, int b0, int nb) {
    if (ph == nullptr || phase < 0 || phase >= h.nph || nb <= 0 || b0 < 0 || b0 > h.batch - nb) return TD_EINVAL;
    if (h.f32 || ph[phase].model != TD_MODEL_WB) return TD_ENOTSUP;
    if (ph[phase].nt <= 0) return TD_EINVAL;
    return TD_OK;
}
// hsddp_touchdown_set: heights [nb][4]; a host source is checked for finite values
inline int td_check_set(const TdHandleInfo& h, const TdPhaseInfo* ph, int phase, int b0, int nb, const double* heights, int src_device) {
    if (heights == nullptr) return TD_EINVAL;
    const int rc = td_check_range(h, ph, phase, b0, nb);
    if (rc != TD_OK) return rc;
    if (!src_device) for (size_t i = 0; i < (size_t)nb * 4; i++) if (!std::isfinite(heights[i])) return TD_EINVAL;
    return TD_OK;
}
// hsddp_touchdown_from_terrain: the `on != 0` rules of hsddp_terrain_set (w_td and `early` play no part here).  A device grid or map cannot be
// read by the host: its values are the caller's responsibility (the lookup clamps the cell, a map index is clamped into [0, n_maps) by the lane).
inline int td_check_terrain(const TdHandleInfo& h, int nx, int ny, int n_maps, double x0, double y0, double cx, double cy, double z_ground,
                            const double* H, const int* map_of, int src_device) {
    if (H == nullptr) return TD_EINVAL;
    if (!std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(z_ground)) return TD_EINVAL;
    if (!(cx > 0.0) || !(cy > 0.0)) return TD_EINVAL;
    if (nx < 1 || nx > 1024 || ny < 1 || ny > 1024 || n_maps < 1 || n_maps > 4096) return TD_EINVAL;
    const size_t cells = (size_t)n_maps * (size_t)nx * (size_t)ny;
    if (cells > ((size_t)1 << 22)) return TD_EINVAL;
    if (!src_device) {
        for (size_t i = 0; i < cells; i++) if (!std::isfinite(H[i])) return TD_EINVAL;
        if (map_of != nullptr) for (int b = 0; b < h.batch; b++) if (map_of[b] < 0 || map_of[b] >= n_maps) return TD_EINVAL;
    }
    if (h.f32) return TD_ENOTSUP;
    return TD_OK;
}

// the grid of one k_td_terrain launch; map_of: null (map 0) or the map of problem b at map_of[b * map_stride]
struct TdGrid {
    const double* H; const int* map_of;
    int map_stride, nx, ny, n_maps;
    double x0, y0, cx, cy, z_ground;
};
// the reference footholds of a phase: rows of 12 doubles, the row of problem b at knot k is b * ref_pb + k (PhaseDev::foot_pos / ref_pb)
struct TdFootRef { const double* foot_pos; int ref_pb, h; };

TD_HD double td_terrain_height(const TdGrid& g, const TdFootRef& r, int b, int leg) {
    const double* p = r.foot_pos + ((size_t)(unsigned)(b * r.ref_pb + r.h)) * 12 + 3 * leg;
    int m = g.map_of != nullptr ? g.map_of[(size_t)b * g.map_stride] : 0;
    m = m < 0 ? 0 : (m >= g.n_maps ? g.n_maps - 1 : m);
    const double fx = fmin(fmax(floor((p[0] - g.x0) / g.cx), 0.0), (double)(g.nx - 1));
    const double fy = fmin(fmax(floor((p[1] - g.y0) / g.cy), 0.0), (double)(g.ny - 1));
    return g.z_ground + g.H[((size_t)m * (size_t)g.ny + (size_t)(int)fy) * (size_t)g.nx + (size_t)(int)fx];
}

#ifdef TOUCHDOWN_HOST_ONLY
// the kernel's loop on the host (tests): out [nph][batch][4]; a phase with on[pi] == 0 is left alone
inline void td_terrain_host(const TdGrid& g, const TdFootRef* refs, const int* on, int nph, int batch, double* out) {
    for (size_t i = 0; i < (size_t)nph * batch * 4; i++) {
        const int leg = (int)(i & 3), b = (int)((i >> 2) % (size_t)batch), pi = (int)((i >> 2) / (size_t)batch);
        if (on[pi]) out[i] = td_terrain_height(g, refs[pi], b, leg);
    }
}
#endif

}  // namespace hs
