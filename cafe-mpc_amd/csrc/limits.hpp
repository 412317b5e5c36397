// Per-problem constraint limits (include/hsddp_limits.h): the argument rules and the loops of the two kernels that write the tables.
//
//   lim_check_set / lim_check_range / lim_check_kappa   the refusal rules, plain functions of the handle's batch, phase count and precision and the
//                  call's arguments: the library applies them before it touches anything, the tests run them as a stand-alone program.
//   LimPack        one launch of k_pack_limits.  user: the table of the caller's rows [batch][12], NaN where nothing is set; res: the RESOLVED table
//                  [nph][batch][12], what problem b uses in phase p; desc: the window's descriptor limits as rows [nph][12].  The launch covers problems
//                  [p0, p0+np).  mode LIM_PACK_FIRST writes NaN outside [b0, b0+nb) and the caller's rows (src, [nb][12]) inside - the first call,
//                  np = batch; LIM_PACK_RANGE writes the caller's rows - later calls, [p0, p0+np) = [b0, b0+nb); LIM_PACK_RESOLVE leaves the user
//                  table as it is - hsddp_reconfigure, np = batch.  Every mode then resolves the covered problems against every phase:
//                  res[p][b][e] = user[b][e] is NaN ? desc[p][e] : user[b][e].  The knot programs read res and decide nothing.
//   lim_pack_item  the work of flat element i (one entry of one problem: one user value, nph resolved ones).
//   LimMu          one launch of k_lim_mu (hsddp_episode_plan_friction): mu of problem b <- kappa * mu_tab[2 * mu_of[b * stride]] (the static
//                  coefficient of the friction row the episode simulates robot b on), in the user table and in every phase's resolved row.
//   lim_mu_item    the work of problem b.
// Compiled for the device in hsddp_lim.hip and for the host by the tests (LIMITS_HOST_ONLY: no HIP headers).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef LIMITS_HOST_ONLY
#define LIM_HD inline
#else
#define LIM_HD __host__ __device__ inline
#endif

namespace hs {

// torque_limit | joint_lb[3] | joint_ub[3] | h_min | mu | jointspeed_lb | jointspeed_ub | pad (hs_types.hpp: LIM_ROW and the LIM_* offsets)
constexpr int LMP_ROW = 12, LMP_TORQUE = 0, LMP_JLB = 1, LMP_JUB = 4, LMP_HMIN = 7, LMP_MU = 8, LMP_JSLB = 9, LMP_JSUB = 10, LMP_PAD = 11;
// return codes of include/hsddp.h (HSDDP_OK, HSDDP_EINVAL, HSDDP_ENOTSUP), repeated so that this header stands alone (limits_host.hpp holds them equal)
enum { LIM_OK = 0, LIM_EINVAL = -1, LIM_ENOTSUP = -4 };
enum { LIM_PACK_FIRST = 0, LIM_PACK_RANGE = 1, LIM_PACK_RESOLVE = 2 };

struct LimHandleInfo { int batch, nph, f32; };

inline int lim_check_range(const LimHandleInfo& H, int b0, int nb) {
    if (nb <= 0 || b0 < 0 || b0 >= H.batch || nb > H.batch - b0) return LIM_EINVAL;
    if (H.f32) return LIM_ENOTSUP;
    return LIM_OK;
}
inline int lim_check_get(const LimHandleInfo& H, int phase, int b0, int nb) {
    if (phase < 0 || phase >= H.nph) return LIM_EINVAL;
    return lim_check_range(H, b0, nb);
}
// rows: [nb][12]; a device source is not read.  Every entry NaN (unset) or finite; torque_limit > 0, mu > 0; lb < ub where both are given; pad ignored
inline int lim_check_set(const LimHandleInfo& H, int b0, int nb, const double* rows, int src_device) {
    if (rows == nullptr) return LIM_EINVAL;
    { const int rc = lim_check_range(H, b0, nb); if (rc) return rc; }
    if (src_device) return LIM_OK;
    for (size_t r = 0; r < (size_t)nb; r++) {
        const double* v = rows + r * LMP_ROW;
        for (int e = 0; e < LMP_PAD; e++) if (std::isinf(v[e])) return LIM_EINVAL;
        if (v[LMP_TORQUE] <= 0.0 || v[LMP_MU] <= 0.0) return LIM_EINVAL;                   // (a NaN passes every comparison below: unset)
        for (int j = 0; j < 3; j++) if (v[LMP_JLB + j] >= v[LMP_JUB + j]) return LIM_EINVAL;
        if (v[LMP_JSLB] >= v[LMP_JSUB]) return LIM_EINVAL;
    }
    return LIM_OK;
}
inline int lim_check_kappa(double kappa) { return (kappa > 0.0 && kappa <= 1.0) ? LIM_OK : LIM_EINVAL; }

struct LimPack { double* user; double* res; const double* src; const double* desc; int batch, nph, b0, nb, p0, np, mode; };

LIM_HD size_t lim_pack_count(const LimPack& W) { return (size_t)W.np * LMP_ROW; }
LIM_HD void lim_pack_item(const LimPack& W, size_t i) {
    const size_t row = i / LMP_ROW; const int e = (int)(i - row * LMP_ROW), b = W.p0 + (int)row;
    const size_t ue = (size_t)b * LMP_ROW + e;
    double u;
    if (W.mode == LIM_PACK_RESOLVE) u = W.user[ue];
    else {
        const bool in = b >= W.b0 && b < W.b0 + W.nb;
        if (in) u = W.src[(size_t)(b - W.b0) * LMP_ROW + e];
        else if (W.mode == LIM_PACK_FIRST) u = NAN;
        else return;      // (a later call covers its own range only: never reached with p0 = b0, np = nb)
        W.user[ue] = u;
    }
    const bool unset = u != u;
    for (int p = 0; p < W.nph; p++) W.res[((size_t)p * W.batch + b) * LMP_ROW + e] = unset ? W.desc[(size_t)p * LMP_ROW + e] : u;
}

struct LimMu { double* user; double* res; const double* mu_tab; const int* mu_of; int stride, batch, nph; double kappa; };

LIM_HD void lim_mu_item(const LimMu& F, int b) {
    const double m = F.kappa * F.mu_tab[2 * (size_t)F.mu_of[(size_t)b * F.stride]];      // one fp64 multiply
    F.user[(size_t)b * LMP_ROW + LMP_MU] = m;
    for (int p = 0; p < F.nph; p++) F.res[((size_t)p * F.batch + b) * LMP_ROW + LMP_MU] = m;
}

#ifdef LIMITS_HOST_ONLY
// the kernels' loops on the host (tests)
inline void lim_pack_host(const LimPack& W) { const size_t n = lim_pack_count(W); for (size_t i = 0; i < n; i++) lim_pack_item(W, i); }
inline void lim_mu_host(const LimMu& F) { for (int b = 0; b < F.batch; b++) lim_mu_item(F, b); }
#endif

}  // namespace hs
