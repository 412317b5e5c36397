// Per-problem tracking references (include/hsddp_refs.h): the packing kernel behind hsddp_set_references.
//
//   RefsPack      one call: the phase's new per-problem storage (dst_*, [batch][h+1][width]), its current storage (cur_*, row stride cur_pb:
//                 0 = shared, h+1 = per problem) and the caller's sources for problems [b0, b0+nb) (src_*, [nb][h+1][width], null = keep).
//                 Problems [p0, p0+np) are written: the whole batch on the phase's first call (every problem starts from the shared rows),
//                 [b0, b0+nb) afterwards.
//   refs_value    the value of one element of segment `seg` (xr, ur, yr, foot_pos, foot_vel, body_pos, ref_contact, rref) at flat index i of
//                 the written range.  The whole-body record rref follows setup_phase (hs_host.hpp) element for element: xr | ur | foot_vel |
//                 ref_contact as doubles | foot_pos - body_pos | zero pad, computed from the NEW raw values.  Compiled for the device here and
//                 for the host by the tests (REFS_PACK_ONLY: this section alone, no HIP headers).
//   k_pack_refs   grid (blocks, 8 segments), 256 threads: each segment is one contiguous destination range, walked with unit stride by
//                 consecutive lanes (coalesced 8-byte loads and stores; the source rows of one segment are contiguous too).
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef REFS_PACK_ONLY
#define REFS_HD inline
#else
#define REFS_HD __host__ __device__ inline
#endif

namespace hs {

enum { RS_XR = 0, RS_UR, RS_YR, RS_FP, RS_FV, RS_BP, RS_RC, RS_RREF, RS_COUNT };

struct RefsPack {
    double *dst[RS_COUNT];                  // RS_RC: int storage (cast), RS_RREF: null unless whole body, RS_YR: null when p = 0
    const double *cur[RS_COUNT - 1];        // current storage of the raw arrays (RS_RC: int)
    const double *src[RS_COUNT - 1];        // caller's rows for problems [b0, b0+nb) or null (RS_RC: int)
    int w[RS_COUNT];                        // widths: n, m, p, 12, 12, 3, 4, 80
    int h1, cur_pb, b0, nb, p0, np;
};

// raw segment s (< RS_RREF) of problem b, knot k, element e: the caller's source inside [b0, b0+nb), the current storage elsewhere
REFS_HD double refs_raw(const RefsPack& R, int s, int b, int k, int e) {
    const int w = R.w[s];
    if (R.src[s] != nullptr && b >= R.b0 && b < R.b0 + R.nb) {
        const size_t i = ((size_t)(b - R.b0) * R.h1 + k) * w + e;
        return s == RS_RC ? (double)((const int*)R.src[s])[i] : R.src[s][i];
    }
    const size_t i = ((size_t)b * R.cur_pb + k) * w + e;
    return s == RS_RC ? (double)((const int*)R.cur[s])[i] : R.cur[s][i];
}

// element i (flat over [p0, p0+np) x (h+1) x w) of segment s
REFS_HD double refs_value(const RefsPack& R, int s, uint32_t i) {
    const uint32_t w = (uint32_t)R.w[s], row = i / w, e = i - row * w, r = row / (uint32_t)R.h1;
    const int b = R.p0 + (int)r, k = (int)(row - r * (uint32_t)R.h1);
    if (s != RS_RREF) return refs_raw(R, s, b, k, (int)e);
    if (e < 36) return refs_raw(R, RS_XR, b, k, (int)e);
    if (e < 48) return refs_raw(R, RS_UR, b, k, (int)e - 36);
    if (e < 60) return refs_raw(R, RS_FV, b, k, (int)e - 48);
    if (e < 64) return refs_raw(R, RS_RC, b, k, (int)e - 60);
    if (e < 76) return refs_raw(R, RS_FP, b, k, (int)e - 64) - refs_raw(R, RS_BP, b, k, (int)(e - 64) % 3);
    return 0.0;
}

// elements of segment s in the written range (0: segment absent)
REFS_HD uint32_t refs_count(const RefsPack& R, int s) {
    return R.dst[s] == nullptr ? 0u : (uint32_t)((size_t)R.np * R.h1 * R.w[s]);
}

#ifdef REFS_PACK_ONLY
// the kernel's loop on the host (tests)
inline void refs_pack_host(const RefsPack& R) {
    for (int s = 0; s < RS_COUNT; s++) {
        const uint32_t n = refs_count(R, s); const size_t o = (size_t)R.p0 * R.h1 * R.w[s];
        for (uint32_t i = 0; i < n; i++) {
            const double v = refs_value(R, s, i);
            if (s == RS_RC) ((int*)R.dst[s])[o + i] = (int)v; else R.dst[s][o + i] = v;
        }
    }
}
#else
// the ranges must fit 32-bit flat indices: the host splits larger calls by problems (refs_max_problems)
__global__ void __launch_bounds__(256) k_pack_refs(RefsPack R) {
    const int s = blockIdx.y;
    const uint32_t n = refs_count(R, s);
    const size_t o = (size_t)R.p0 * R.h1 * R.w[s];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double v = refs_value(R, s, i);
        if (s == RS_RC) ((int*)R.dst[s])[o + i] = (int)v; else R.dst[s][o + i] = v;
    }
}
#endif

}  // namespace hs
