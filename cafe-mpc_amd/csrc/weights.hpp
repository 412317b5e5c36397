// Per-problem cost-weight scales (include/hsddp_weights.h): the argument rules and the packing kernel behind hsddp_weights_set.
//
//   ws_check_set / ws_check_range   the refusal rules, plain functions of the handle's batch and precision and the call's arguments: the library
//                                   applies them before it touches anything, the tests run them as a stand-alone program.
//   WsPack        one call: the table (dst, [batch][84]), the caller's rows for problems [b0, b0+nb) (src, [nb][84]: a device source or the staged
//                 copy of a host one) and the rows [p0, p0+np) that are written - the whole batch on the first call, with 1.0 outside the caller's
//                 range, [b0, b0+nb) afterwards.
//   ws_value      the value of flat element i of the written range.  Compiled for the device here and for the host by the tests
//                 (WEIGHTS_HOST_ONLY: no HIP headers).
//   k_pack_weights   (hsddp_pw.hip) 256 threads, consecutive lanes on consecutive doubles (coalesced 8-byte loads and stores): dst[i] = ws_value(i).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef WEIGHTS_HOST_ONLY
#define WS_HD inline
#else
#define WS_HD __host__ __device__ inline
#endif

namespace hs {

constexpr int WSP_ROW = 84, WSP_R = 36, WSP_QF = 48;      // sq[36] | sr[12] | sqf[36] (hs_types.hpp: WS_ROW, WS_R, WS_QF)
// return codes of include/hsddp.h (HSDDP_OK, HSDDP_EINVAL, HSDDP_ENOTSUP), repeated so that this header stands alone (weights_host.hpp holds them equal)
enum { WS_OK = 0, WS_EINVAL = -1, WS_ENOTSUP = -4 };

struct WsHandleInfo { int batch, f32; };

inline int ws_check_range(const WsHandleInfo& H, int b0, int nb) {
    if (nb <= 0 || b0 < 0 || b0 >= H.batch || nb > H.batch - b0) return WS_EINVAL;
    if (H.f32) return WS_ENOTSUP;
    return WS_OK;
}
// scales: [nb][84]; a device source is not read
inline int ws_check_set(const WsHandleInfo& H, int b0, int nb, const double* scales, int src_device) {
    if (scales == nullptr) return WS_EINVAL;
    { const int rc = ws_check_range(H, b0, nb); if (rc) return rc; }
    if (src_device) return WS_OK;
    for (size_t r = 0; r < (size_t)nb; r++) for (int e = 0; e < WSP_ROW; e++) {
        const double v = scales[r * WSP_ROW + e];
        if (!std::isfinite(v)) return WS_EINVAL;
        if (e >= WSP_R && e < WSP_QF) { if (!(v > 0.0)) return WS_EINVAL; }      // sr > 0: luu has to stay positive definite
        else if (!(v >= 0.0)) return WS_EINVAL;                                 // sq, sqf >= 0
    }
    return WS_OK;
}

struct WsPack { double* dst; const double* src; int b0, nb, p0, np; };

WS_HD size_t ws_count(const WsPack& W) { return (size_t)W.np * WSP_ROW; }
WS_HD double ws_value(const WsPack& W, size_t i) {
    const size_t row = i / WSP_ROW; const int e = (int)(i - row * WSP_ROW), b = W.p0 + (int)row;
    if (b >= W.b0 && b < W.b0 + W.nb) return W.src[(size_t)(b - W.b0) * WSP_ROW + e];
    return 1.0;
}

#ifdef WEIGHTS_HOST_ONLY
// the kernel's loop on the host (tests)
inline void ws_pack_host(const WsPack& W) {
    const size_t n = ws_count(W), o = (size_t)W.p0 * WSP_ROW;
    for (size_t i = 0; i < n; i++) W.dst[o + i] = ws_value(W, i);
}
#endif

}  // namespace hs
