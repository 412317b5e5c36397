// Closed-loop rollout of a solved whole-body policy from perturbed initial states, on LANE QUADS (include/hsddp_sim.h).
//
// One quad of lanes per (problem, sample), lane = leg as in wb_quad.hpp.  The quad keeps the state in registers and walks the first
// n_steps control knots of the handle in a loop:
//     u = Ubar_k + K_k (x - Xbar_k) ;  x <- x + dt (v, qdd(x, u))          (the knot step of the rollout: WBM.cpp:17-57, 368-424)
//     at the end of a phase, if the window goes on:  v <- v+ of the impact on the feet that touch down   (WBM.cpp:178-206, 427-456)
// which is what the single-shooting chain of hsddp_hybrid_rollout(eps = 0, MS = 0) computes from the same initial state - without the costs,
// defects and constraint values, without a write to the handle, and for R samples per problem.  No barrier; LDS only as a lane-private parking
// place of the loop-carried values across the contact solve.
//
// The sixteen quads of a wave are consecutive (problem, sample) pairs, sample fastest: with R a multiple of 16 a wave holds sixteen samples
// of ONE problem, and Xbar, Ubar and the 432 gains of a knot are the same addresses in every quad (each line is touched once per wave).
//
// wbs_contact_dynamics is the state -> (qdd, lambda) part of wbq_rollout_knot (wb_quad.hpp: composite inertias, bias forces, foot Jacobian,
// block factor, block contact solve) COPIED here on purpose: sharing it would mean editing wbq_rollout_knot, and k_rollout_quad has to keep
// compiling to exactly what it compiles to now.  About 300 lines are duplicated; a change to the dynamics there has to be made here too
// (tests/test_sim_host.py and tests/test_sim_gpu.py hold the two against the oracle and against each other).  The copy takes the contact set,
// the mode and the Gram damping as wave-uniform arguments, because the impact is the same solve in another mode (wb_kkt_direct, wb_knot.hpp):
//     mode 0 (forwardDynamics):  y = L^-1 (tau - h), lam = G^-1 (-X^T y - gam), qdd = L^-T (y + X lam), damping 1e-12
//     mode 1 (impulseDynamics):  contact set = the feet that touch down, lam = G^-1 (-Jc v), v+ = v + L^-T X lam, damping 0
// (Jc v of a foot is its velocity, which the bias pass leaves behind anyway; y = 0, so no product with L^T is needed.)
#pragma once
#include "wb_quad.hpp"
#include "sim_pick.hpp"

namespace hs {

#ifdef HS_HOST_EMU
inline int wbs_uniform(int v) { return v; }
#else
HD int wbs_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }      // a value every lane of the wave holds alike: into a scalar register
#endif
#ifndef SIM_PREFETCH
// SIM_PREFETCH 1: the next knot's Xbar / Ubar / K rows (they do not depend on the state) are fetched ahead of the current knot's contact solve
// instead of at the head of their own knot.  Measured on the MI355X, config 3, 4 096 problems x 16 samples x 200 steps, before the loop-carried
// values were parked in LDS: 49.0 ms against 13.5 ms - the 129 doubles held across the contact solve pushed the kernel from 304 to 1 344 bytes of
// scratch per lane, and the spill traffic costs far more than the exposed round trip of loads that mostly hit the L2 (a build that reads one
// gain per torque instead of 108 put that round trip at 1.9 ms of the 13.5).  With the parking it is still 1 064 bytes (make resources).  Off.
#define SIM_PREFETCH 0
#endif
#ifndef HS_HOST_EMU
// QD whose lane index is laundered through an empty asm at every use: nothing derived from it (leg signs, link inertias, selection masks) is
// loop-invariant to the compiler, which would otherwise compute all of it once in front of the step loop and hold it in registers across the
// whole knot (HS_PHASE does the same with tid, hs_common.hpp)
struct QS : QD {
    static HD int lane() { int l = threadIdx.x & 3; asm volatile("" : "+v"(l)); return l; }
    static HD S legc(double a, double b, double c, double d) { const int l = lane(); return l == 0 ? a : l == 1 ? b : l == 2 ? c : d; }
    template <class PT> static HD S ld(PT p, size_t off, int stride) { return p[off + (size_t)(lane() * stride)]; }
    template <class PT> static HD void st(PT p, size_t off, int stride, S x) { p[off + (size_t)(lane() * stride)] = x; }
    template <class PT> static HD void st0(PT p, size_t off, S x) { if (lane() == 0) p[off] = x; }
};
#endif
template <class Q, class S> HD S wbs_abs(const S& a) { return Q::sel(Q::gt(S(0.0), a), -a, a); }
template <class Q, class S> HD S wbs_max(const S& a, const S& b) { return Q::sel(Q::gt(b, a), b, a); }
template <class Q, class S> HD S wbs_qmax(const S& a) { return -Q::vmin(-a); }      // maximum over the four lanes of the quad

// Contact dynamics of one state on a lane quad.  cmask: bit l = leg l is in the contact set; mode, damping, bg_alpha: see the head of the file
// (all four wave-uniform).  out_b (6, replicated) / out_l (the lane's leg): mode 0 the accelerations qdd, mode 1 the velocities after the impact.
// lam_out (optional, one V3<S>*): the contact force of the lane's foot, world axes - the multiplier of the solve; zero for a leg outside the contact
// set.  It is a parameter PACK so that a call without it instantiates the function it instantiated before the output existed, signature and body:
// as a defaulted pointer argument it moved the register allocation of every caller (k_sim_quad: 24 -> 0 B of scratch - welcome, but not this
// change's business, which has to leave the existing kernels what they are).  The store keeps its null test although no caller passes null: with it
// the three kernels that take the force compile to 0 / 76 / 0 B of scratch per lane, without it to 40 / 148 / 44 (make resources).
// Unilateral contact (include/hsddp_contact.h): the one pack element of a solve whose contact flag is the LANE's own.  cl: 1 if the lane's foot is in
// the contact set (cmask is not read); the solve hands back the force as above, and the height and vertical velocity of the lane's foot point at the
// state it was given (qb[2] + rW.z, fvel.z - computed for the bias pass anyway).  The calls without it instantiate what they instantiated before.
template <class S> struct WbsUniIO { S cl, pz, wz; V3<S> lam; };
template <class T> struct wbs_is_uni_io { static constexpr bool value = false; };
template <class S> struct wbs_is_uni_io<WbsUniIO<S>> { static constexpr bool value = true; };
template <class Q, class S, class... LO> HD S wbs_lane_flag(int cmask, LO*...) { return Q::legc((cmask & 1) ? 1.0 : 0.0, (cmask & 2) ? 1.0 : 0.0, (cmask & 4) ? 1.0 : 0.0, (cmask & 8) ? 1.0 : 0.0); }
template <class Q, class S> HD S wbs_lane_flag(int, WbsUniIO<S>* io) { return io->cl; }
// Terrain (include/hsddp_terrain.h): the same exchange plus the x and y of the lane's foot point (fpos, computed for the bias pass anyway), which the
// height lookup needs.  An element type of its own, so that a solve with WbsUniIO instantiates what it instantiated before this one existed.
template <class S> struct WbsTerIO { S cl, pz, wz, px, py; V3<S> lam; };
template <class T> struct wbs_is_ter_io { static constexpr bool value = false; };
template <class S> struct wbs_is_ter_io<WbsTerIO<S>> { static constexpr bool value = true; };
template <class Q, class S> HD S wbs_lane_flag(int, WbsTerIO<S>* io) { return io->cl; }
// Plant-model mismatch (include/hsddp_plant.h): the exchange of WbsTerIO plus `row`, the quad's row of the plant table (HSDDP_PLANT_ROW doubles).  A solve
// with this element reads the trunk's and the links' inertias from the row WHERE IT USES THEM (the trunk's ten values at the IT sum and at the trunk's own
// link_force, the lane's three link scales at the composite inertias and again at the bias pass) instead of the literals; gain and friction are the
// walk's business.  An element type of its own again: every solve without it instantiates what it instantiated before this one existed.
template <class S> struct WbsPlantIO { S cl, pz, wz, px, py; V3<S> lam; const double* row; };
template <class T> struct wbs_is_plant_io { static constexpr bool value = false; };
template <class S> struct wbs_is_plant_io<WbsPlantIO<S>> { static constexpr bool value = true; };
template <class Q, class S> HD S wbs_lane_flag(int, WbsPlantIO<S>* io) { return io->cl; }
template <class... LO> HD const double* wbs_plant_row(LO*...) { return nullptr; }
template <class S> HD const double* wbs_plant_row(WbsPlantIO<S>* io) { return io->row; }
// Coulomb friction (include/hsddp_friction.h): the exchange of WbsTerIO plus the lane's friction COLUMN, `col` with `stride` doubles between its slots - on
// the device the lane's own column of the parked LDS block, so that nothing of it sits in registers across the solve's register peak.  Slots the solve
// reads: SL (1: the lane's foot is in the sliding set), FRESH (1: it joined the set in this substep), NF (the lagged normal force), TX / TY (the direction
// of a fresh foot's friction).  Slots it writes: EFF (1: this solve treated the foot as sliding - 0 for a foot that re-sticks), FX / FY (the friction force
// it applied), WX / WY (the tangential velocity of the foot point at the state it was given).  mur: the sample's row (mu_s, mu_k) of the table; vstick:
// the re-stick speed.  A sliding foot keeps its z row alone: its x and y columns of X, its right-hand side and its multipliers are masked, its Gram block
// gets the identity on those two diagonals, and the known force enters tau - h through J^T f_t.  An element type of its own: every other solve
// instantiates what it did before.
enum { FRIC_SL = 0, FRIC_FRESH, FRIC_NF, FRIC_TX, FRIC_TY, FRIC_FIRST, FRIC_NONSET, FRIC_NSLIDE, FRIC_NRESTICK, FRIC_VMAX, FRIC_DIST, FRIC_EFF, FRIC_FX, FRIC_FY, FRIC_WX, FRIC_WY, FRIC_SLOTS };
template <class S> struct WbsFricIO { S cl, pz, wz, px, py; V3<S> lam; S* col; int stride; const double* mur; double vstick; };
template <class T> struct wbs_is_fric_io { static constexpr bool value = false; };
template <class S> struct wbs_is_fric_io<WbsFricIO<S>> { static constexpr bool value = true; };
template <class Q, class S> HD S wbs_lane_flag(int, WbsFricIO<S>* io) { return io->cl; }
#ifdef HS_HOST_EMU
inline Q4 wbs_sqrt(const Q4& x) { return Q4(std::sqrt(x.v[0]), std::sqrt(x.v[1]), std::sqrt(x.v[2]), std::sqrt(x.v[3])); }
template <class S> inline S& wbs_fric_slot(WbsFricIO<S>* io, int i) { return io->col[i * io->stride]; }
#else
HD double wbs_sqrt(double x) { return ::sqrt(x); }
// the offset is laundered: every use is a read of LDS where it stands, never a value the compiler carries from an earlier one
template <class S> HD S& wbs_fric_slot(WbsFricIO<S>* io, int i) { int o = i * io->stride; asm volatile("" : "+v"(o)); return io->col[o]; }
#endif
// What a sliding solve needs, formed where fvel is known: the effective flag and the friction force.  A fresh foot is pushed along its stored
// direction; any other sliding foot against its tangential velocity if that is faster than vstick, and re-sticks otherwise (selects, no products with a
// flag: the direction of a foot at rest is 0 / 0).  m0: 1 in mode 0, 0 in mode 1 - an impact holds every foot with three rows.
template <class Q, class S> HD void wbs_fric_force(WbsFricIO<S>* io, const V3<S>& fvel, double m0) {
    const S zero = S(0.0), one = S(1.0);
    const S wt = wbs_sqrt(fvel.x * fvel.x + fvel.y * fvel.y);
    const typename Q::B sliding = Q::gt(io->cl * wbs_fric_slot(io, FRIC_SL) * m0, S(0.5)), isfresh = Q::gt(wbs_fric_slot(io, FRIC_FRESH), S(0.5)), moving = Q::gt(wt, S(io->vstick));
    const S eff = Q::sel(sliding, Q::sel(isfresh, one, Q::sel(moving, one, zero)), zero);
    const S rw = Q::rcp(wt), mag = Q::ld(io->mur, 1, 0) * wbs_fric_slot(io, FRIC_NF);
    const S dx = Q::sel(isfresh, wbs_fric_slot(io, FRIC_TX), -(fvel.x * rw)), dy = Q::sel(isfresh, wbs_fric_slot(io, FRIC_TY), -(fvel.y * rw));
    const typename Q::B act = Q::gt(eff, S(0.5));
    wbs_fric_slot(io, FRIC_EFF) = eff; wbs_fric_slot(io, FRIC_FX) = Q::sel(act, mag * dx, zero); wbs_fric_slot(io, FRIC_FY) = Q::sel(act, mag * dy, zero);
    wbs_fric_slot(io, FRIC_WX) = fvel.x; wbs_fric_slot(io, FRIC_WY) = fvel.y;
}
template <class S, class... LO> HD WbsFricIO<S>* wbs_fric_ptr(LO*...) { return nullptr; }
template <class S> HD WbsFricIO<S>* wbs_fric_ptr(WbsFricIO<S>* io) { return io; }
// rbi_link with a mass that is a value of the lane (wb_quad.hpp's takes a literal): the same operations in the same order
template <class S> HD RBI<S> wbs_plant_link(S m, S cx, S cy, S cz, S ixx, S ixy, S ixz, S iyy, S iyz, S izz) {
    RBI<S> R; R.m = m; R.h = {m * cx, m * cy, m * cz};
    const S cc = cx * cx + cy * cy + cz * cz;
    R.I = {ixx + m * (cc - cx * cx), ixy - m * (cx * cy), ixz - m * (cx * cz), iyy + m * (cc - cy * cy), iyz - m * (cy * cz), izz + m * (cc - cz * cz)};
    return R;
}
// wbs_pick<true>(a, b) is a, wbs_pick<false>(a, b) is b: a solve without the plant keeps every statement it had, where it had it
template <bool FIRST, class T> HD const T& wbs_pick(const T& a, const T& b) { if constexpr (FIRST) return a; else return b; }
// the trunk of a plant row about the trunk origin: entries 0 .. 9 (mass, CoM, inertia about the CoM), the same address in every lane
template <class Q, class S> HD RBI<S> wbs_plant_trunk(const double* pr) {
    return wbs_plant_link<S>(Q::ld(pr, 0, 0), Q::ld(pr, 1, 0), Q::ld(pr, 2, 0), Q::ld(pr, 3, 0), Q::ld(pr, 4, 0), Q::ld(pr, 5, 0), Q::ld(pr, 6, 0), Q::ld(pr, 7, 0), Q::ld(pr, 8, 0), Q::ld(pr, 9, 0));
}
// the lane's three links with mass and CoM inertia scaled by entries 10 + 3 leg + (0, 1, 2) of the row; CoM and geometry stay
template <class Q, class S> HD void wbs_plant_leg_links(const double* pr, const S& sy, RBI<S>& Iab, RBI<S>& Ith, RBI<S>& Ikn) {
    const S zero = S(0.0), sa = Q::ld(pr, 10, 3), sh = Q::ld(pr, 11, 3), sk = Q::ld(pr, 12, 3);
    Iab = wbs_plant_link<S>(sa * 0.54, zero, sy * 0.036, zero, sa * 0.000381, sa * (sy * 0.000058), sa * 0.00000045, sa * 0.000560, sa * (sy * 0.00000095), sa * 0.000444);
    Ith = wbs_plant_link<S>(sh * 0.634, zero, sy * 0.016, S(-0.02), sh * 0.001983, sh * (sy * 0.000245), sh * 0.000013, sh * 0.002103, sh * (sy * 0.0000015), sh * 0.000408);
    Ikn = wbs_plant_link<S>(sk * 0.064, zero, zero, S(-0.061), sk * 0.000245, zero, zero, sk * 0.000248, zero, sk * 0.000006);
}
template <class Q, class S = typename Q::S, class... LO>
HD void wbs_contact_dynamics(const ModelDev& md, int cmask, int mode, double damping, double bg_alpha, const S (&qb)[6], const S (&vb)[6], const S (&ql)[3],
                             const S (&vl_)[3], const S (&ul)[3], S (&out_b)[6], V3<S>& out_l, LO*... lam_out) {
    const S zero = S(0.0);
    const double m0 = mode == 0 ? 1.0 : 0.0, m1 = 1.0 - m0;      // (1.0 * x is x: mode 0 is the arithmetic of wbq_rollout_knot)
    const S sx = Q::legc(1.0, 1.0, -1.0, -1.0), sy = Q::legc(1.0, -1.0, 1.0, -1.0);
    const double cps = md.cpsi_dyn, sps = md.spsi_dyn;      // every term of the rollout is a Pinocchio-equivalent one (quirk xii)
    Base3<S> T; S ca, sa, ch, sh, ck, sk;
    {   // the three base angles: lane l < 3 evaluates angle 3 + l (lane 3 repeats the last), the quad reads the results
        const S ang = Q::legc(1, 0, 0, 0) * qb[3] + Q::legc(0, 1, 0, 0) * qb[4] + Q::legc(0, 0, 1, 1) * qb[5];
        S sb, cb_; Q::sincos(ang, sb, cb_);
        T.s3 = Q::template get<0>(sb); T.c3 = Q::template get<0>(cb_); T.s4 = Q::template get<1>(sb); T.c4 = Q::template get<1>(cb_); T.s5 = Q::template get<2>(sb); T.c5 = Q::template get<2>(cb_);
    }
    Q::sincos(ql[0], sa, ca); Q::sincos(ql[1], sh, ch); Q::sincos(ql[2], sk, ck);
    const V3<S> pa = {sx * 0.19, sy * 0.049, S(0.0)}, ph = {S(0.0), sy * 0.062, S(0.0)}, pk = {S(0.0), S(0.0), S(-0.209)};

    // ---- composite inertias, leg -> trunk (frames: K shank, H thigh, A abad, B trunk; v_H = Ry(qk) v_K, v_A = Rz(psi) Ry(qh) v_H, v_B = Rx(qa) v_A)
    constexpr bool PLANT = (wbs_is_plant_io<LO>::value || ...);      // (hsddp_plant.h) the inertias come from the quad's plant row
    RBI<S> pA, pH, pK;      // (plant only) the lane's three links of the row; wbs_pick takes them instead of the literals' links
    if constexpr (PLANT) wbs_plant_leg_links<Q, S>(wbs_plant_row(lam_out...), sy, pA, pH, pK);
    const RBI<S> IK = wbs_pick<PLANT>(pK, rbi_link<S>(0.064, zero, zero, S(-0.061), S(0.000245), zero, zero, S(0.000248), zero, S(0.000006)));
    RBI<S> IH = wbs_pick<PLANT>(pH, rbi_link<S>(0.634, zero, sy * 0.016, S(-0.02), S(0.001983), sy * 0.000245, S(0.000013), S(0.002103), sy * 0.0000015, S(0.000408)));
    IH = rbi_add(IH, rbi_shift(IK.m, rot<1>(ck, sk, IK.h), sym_rot<1>(ck, sk, IK.I), pk));
    RBI<S> IA = wbs_pick<PLANT>(pA, rbi_link<S>(0.54, zero, sy * 0.036, zero, S(0.000381), sy * 0.000058, S(0.00000045), S(0.000560), sy * 0.00000095, S(0.000444)));
    IA = rbi_add(IA, rbi_shift(IH.m, rot<2>(S(cps), S(sps), rot<1>(ch, sh, IH.h)), sym_rot<2>(S(cps), S(sps), sym_rot<1>(ch, sh, IH.I)), ph));
    const RBI<S> IBl = rbi_shift(IA.m, rot<0>(ca, sa, IA.h), sym_rot<0>(ca, sa, IA.I), pa);
    // whole robot about the trunk origin: trunk + the four legs (sums over the quad)
    RBI<S> IT;
    IT.m = Q::sum(IBl.m) + 3.3; IT.h = {Q::sum(IBl.h.x), Q::sum(IBl.h.y), Q::sum(IBl.h.z)};
    IT.I = {Q::sum(IBl.I.xx) + 0.011253, Q::sum(IBl.I.xy), Q::sum(IBl.I.xz), Q::sum(IBl.I.yy) + 0.036203, Q::sum(IBl.I.yz), Q::sum(IBl.I.zz) + 0.042673};
    if constexpr (PLANT) {      // the row's trunk instead of the literals' (which the compiler drops)
        const RBI<S> It0 = wbs_plant_trunk<Q, S>(wbs_plant_row(lam_out...));
        IT.m = Q::sum(IBl.m) + It0.m; IT.h = {Q::sum(IBl.h.x) + It0.h.x, Q::sum(IBl.h.y) + It0.h.y, Q::sum(IBl.h.z) + It0.h.z};
        IT.I = {Q::sum(IBl.I.xx) + It0.I.xx, Q::sum(IBl.I.xy) + It0.I.xy, Q::sum(IBl.I.xz) + It0.I.xz, Q::sum(IBl.I.yy) + It0.I.yy, Q::sum(IBl.I.yz) + It0.I.yz, Q::sum(IBl.I.zz) + It0.I.zz};
    }
    // ---- mass-matrix blocks of the leg: D (3x3, joints abad / hip / knee) and Ct[c][j] = M(base joint c, leg joint j)
    S Ct[6][3], d_aa, d_ha, d_hh, d_ka, d_kh, d_kk;
    {
        // knee: unit acceleration about y of K
        V3<S> n = {IK.I.xy, IK.I.yy, IK.I.yz}, f = {IK.h.z, zero, -IK.h.x};
        d_kk = n.y;
        f = rot<1>(ck, sk, f); n = rot<1>(ck, sk, n); force_shift(pk, n, f);                              // -> H
        d_kh = n.y;
        f = rot<2>(S(cps), S(sps), rot<1>(ch, sh, f)); n = rot<2>(S(cps), S(sps), rot<1>(ch, sh, n)); force_shift(ph, n, f);      // -> A
        d_ka = n.x;
        f = rot<0>(ca, sa, f); n = rot<0>(ca, sa, n); force_shift(pa, n, f);                              // -> B
        S t[6]; base_walk(T, f, n, t);
        _Pragma("unroll") for (int c = 0; c < 6; c++) Ct[c][2] = t[c];
    }
    {
        V3<S> n = {IH.I.xy, IH.I.yy, IH.I.yz}, f = {IH.h.z, zero, -IH.h.x};                               // hip: about y of H
        d_hh = n.y;
        f = rot<2>(S(cps), S(sps), rot<1>(ch, sh, f)); n = rot<2>(S(cps), S(sps), rot<1>(ch, sh, n)); force_shift(ph, n, f);
        d_ha = n.x;
        f = rot<0>(ca, sa, f); n = rot<0>(ca, sa, n); force_shift(pa, n, f);
        S t[6]; base_walk(T, f, n, t);
        _Pragma("unroll") for (int c = 0; c < 6; c++) Ct[c][1] = t[c];
    }
    {
        V3<S> n = {IA.I.xx, IA.I.xy, IA.I.xz}, f = {zero, -IA.h.z, IA.h.y};                               // abad: about x of A
        d_aa = n.x;
        f = rot<0>(ca, sa, f); n = rot<0>(ca, sa, n); force_shift(pa, n, f);
        S t[6]; base_walk(T, f, n, t);
        _Pragma("unroll") for (int c = 0; c < 6; c++) Ct[c][0] = t[c];
    }
    // ---- base block B (6x6, replicated): unit accelerations of the base joints seen in trunk axes, force of the WHOLE robot, walked back
    S Bm[21];
    {
        V3<S> acc[6][2];      // [c][0] angular, [c][1] linear
        const V3<S> z3 = {zero, zero, zero};
        const V3<S> ex = {S(1.0), zero, zero}, ey = {zero, S(1.0), zero}, ez = {zero, zero, S(1.0)};
        auto w2b = [&](const V3<S>& w) { return rotT<0>(T.c5, T.s5, rotT<1>(T.c4, T.s4, rotT<2>(T.c3, T.s3, w))); };
        acc[0][0] = z3; acc[0][1] = w2b(ex); acc[1][0] = z3; acc[1][1] = w2b(ey); acc[2][0] = z3; acc[2][1] = w2b(ez);
        acc[3][0] = rotT<0>(T.c5, T.s5, rotT<1>(T.c4, T.s4, ez)); acc[3][1] = z3;
        acc[4][0] = rotT<0>(T.c5, T.s5, ey); acc[4][1] = z3;
        acc[5][0] = ex; acc[5][1] = z3;
        _Pragma("unroll")
        for (int c = 0; c < 6; c++) {
            V3<S> n, f; rbi_apply(IT, acc[c][0], acc[c][1], n, f);
            S t[6]; base_walk(T, f, n, t);
            _Pragma("unroll") for (int i = c; i < 6; i++) Bm[tri(i, c)] = t[i];
        }
    }
    // ---- bias forces: one Newton-Euler pass down and up the leg with the knot's velocities, zero acceleration, gravity as a base acceleration
    S hl[3], hb[6]; V3<S> fpos, fvel, jdv;
    V3<S> rB;      // foot relative to the trunk origin, trunk axes (for the Jacobian below)
    V3<S> dA, dH;  // foot relative to the abad origin (trunk axes after Rx: see below) / hip origin, A axes
    {
        V3<S> om = {zero, zero, zero}, aa = om, vl = {vb[0], vb[1], vb[2]}, al = {zero, zero, S(GRAV)};
        auto revj = [&](auto AXT, const S& c, const S& s, const S& qd, V3<S>& om_, V3<S>& vl_2, V3<S>& aa_, V3<S>& al_) {
            constexpr int AX = decltype(AXT)::value;
            V3<S> o = rotT<AX>(c, s, om_), v = rotT<AX>(c, s, vl_2), a2 = rotT<AX>(c, s, aa_), a1 = rotT<AX>(c, s, al_);
            if (AX == 0) { o.x = o.x + qd; a2.y = a2.y + o.z * qd; a2.z = a2.z - o.y * qd; a1.y = a1.y + v.z * qd; a1.z = a1.z - v.y * qd; }
            if (AX == 1) { o.y = o.y + qd; a2.x = a2.x - o.z * qd; a2.z = a2.z + o.x * qd; a1.x = a1.x - v.z * qd; a1.z = a1.z + v.x * qd; }
            if (AX == 2) { o.z = o.z + qd; a2.x = a2.x + o.y * qd; a2.y = a2.y - o.x * qd; a1.x = a1.x + v.y * qd; a1.y = a1.y - v.x * qd; }
            om_ = o; vl_2 = v; aa_ = a2; al_ = a1;
        };
        using A0 = IC<0>; using A1 = IC<1>; using A2 = IC<2>;
        revj(A2{}, T.c3, T.s3, vb[3], om, vl, aa, al); revj(A1{}, T.c4, T.s4, vb[4], om, vl, aa, al); revj(A0{}, T.c5, T.s5, vb[5], om, vl, aa, al);
        // force of a link: I a + v x* I v with the link's inertia about its origin
        auto link_force = [&](const RBI<S>& I, const V3<S>& o, const V3<S>& v, const V3<S>& a2, const V3<S>& a1, V3<S>& n, V3<S>& f) {
            const V3<S> hl_ = scale(I.m, v) + cross(o, I.h);                 // linear momentum  m v + om x h
            const V3<S> ha = symmul(I.I, o) + cross(I.h, v);                 // angular momentum about the origin
            rbi_apply(I, a2, a1, n, f);
            f = f + cross(o, hl_);
            n = n + cross(o, ha) + cross(v, hl_);
        };
        // trunk (own link only; its wrench joins the legs' in the quad sum, so only lane 0's copy is counted)
        RBI<S> pT, qA, qH, qK;      // (plant only) the trunk and the lane's links, formed again from the row: cheaper than carrying them from the composite pass
        if constexpr (PLANT) { pT = wbs_plant_trunk<Q, S>(wbs_plant_row(lam_out...)); wbs_plant_leg_links<Q, S>(wbs_plant_row(lam_out...), sy, qA, qH, qK); }
        const RBI<S> Itr = wbs_pick<PLANT>(pT, rbi_link<S>(3.3, zero, zero, zero, S(0.011253), zero, zero, S(0.036203), zero, S(0.042673)));
        V3<S> nb, fb; link_force(Itr, om, vl, aa, al, nb, fb);
        const S l0 = Q::legc(1.0, 0.0, 0.0, 0.0);
        nb = scale(l0, nb); fb = scale(l0, fb);
        // down the leg
        V3<S> o1 = om, a1 = aa, v1 = vl + cross(om, pa), l1 = al + cross(aa, pa);
        revj(A0{}, ca, sa, vl_[0], o1, v1, a1, l1);
        const RBI<S> Iab = wbs_pick<PLANT>(qA, rbi_link<S>(0.54, zero, sy * 0.036, zero, S(0.000381), sy * 0.000058, S(0.00000045), S(0.000560), sy * 0.00000095, S(0.000444)));
        V3<S> n1, f1; link_force(Iab, o1, v1, a1, l1, n1, f1);
        V3<S> o2 = o1, a2 = a1, v2 = v1 + cross(o1, ph), l2 = l1 + cross(a1, ph);
        o2 = rotT<2>(S(cps), S(sps), o2); v2 = rotT<2>(S(cps), S(sps), v2); a2 = rotT<2>(S(cps), S(sps), a2); l2 = rotT<2>(S(cps), S(sps), l2);
        revj(A1{}, ch, sh, vl_[1], o2, v2, a2, l2);
        const RBI<S> Ith = wbs_pick<PLANT>(qH, rbi_link<S>(0.634, zero, sy * 0.016, S(-0.02), S(0.001983), sy * 0.000245, S(0.000013), S(0.002103), sy * 0.0000015, S(0.000408)));
        V3<S> n2, f2; link_force(Ith, o2, v2, a2, l2, n2, f2);
        V3<S> o3 = o2, a3 = a2, v3 = v2 + cross(o2, pk), l3 = l2 + cross(a2, pk);
        revj(A1{}, ck, sk, vl_[2], o3, v3, a3, l3);
        V3<S> n3, f3; link_force(IK, o3, v3, a3, l3, n3, f3);
        // foot point (0, 0, -0.195) in K: velocity, classical acceleration, position
        const V3<S> rf = {zero, zero, S(-0.195)};
        const V3<S> vp = v3 + cross(o3, rf), ap = l3 + cross(a3, rf) + cross(o3, vp);
        auto up = [&](V3<S> w) {      // K -> world
            w = rot<1>(ck, sk, w); w = rot<1>(ch, sh, w); w = rot<2>(S(cps), S(sps), w); w = rot<0>(ca, sa, w);
            w = rot<0>(T.c5, T.s5, w); w = rot<1>(T.c4, T.s4, w); w = rot<2>(T.c3, T.s3, w); return w;
        };
        fvel = up(vp); jdv = up(ap); jdv.z = jdv.z - GRAV;
        const V3<S> rK = rot<1>(ck, sk, rf);                            // foot relative to the knee origin, H axes
        const V3<S> rH = pk + rK;                                       // ... relative to the hip origin, H axes
        dH = rot<2>(S(cps), S(sps), rot<1>(ch, sh, rH));                // ... relative to the hip origin, A axes
        const V3<S> rA = ph + dH;                                       // ... relative to the abad origin, A axes
        dA = rot<0>(ca, sa, rA);                                        // ... relative to the abad origin, trunk axes
        rB = pa + dA;
        const V3<S> rW = rot<2>(T.c3, T.s3, rot<1>(T.c4, T.s4, rot<0>(T.c5, T.s5, rB)));
        fpos = V3<S>{qb[0], qb[1], qb[2]} + rW;
        // back up the leg
        hl[2] = n3.y;
        V3<S> fu = rot<1>(ck, sk, f3), nu = rot<1>(ck, sk, n3);
        f2 = f2 + fu; n2 = n2 + nu + cross(pk, fu);
        hl[1] = n2.y;
        fu = rot<2>(S(cps), S(sps), rot<1>(ch, sh, f2)); nu = rot<2>(S(cps), S(sps), rot<1>(ch, sh, n2));
        f1 = f1 + fu; n1 = n1 + nu + cross(ph, fu);
        hl[0] = n1.x;
        fu = rot<0>(ca, sa, f1); nu = rot<0>(ca, sa, n1);
        fb = fb + fu; nb = nb + nu + cross(pa, fu);
        fb = {Q::sum(fb.x), Q::sum(fb.y), Q::sum(fb.z)}; nb = {Q::sum(nb.x), Q::sum(nb.y), Q::sum(nb.z)};
        base_walk(T, fb, nb, hb);
    }
    // ---- foot Jacobian of the leg, world axes: Ja (3 x 3 over abad, hip, knee), Jb (3 x 6 over the base joints) - geometric form axis x arm
    const S cl = wbs_lane_flag<Q, S>(cmask, lam_out...);      // contact flag of the lane's leg
    M33<S> Ja; S Jb[3][6];
    {
        auto b2w = [&](const V3<S>& w) { return rot<2>(T.c3, T.s3, rot<1>(T.c4, T.s4, rot<0>(T.c5, T.s5, w))); };
        const V3<S> ex = {S(1.0), zero, zero}, ey = {zero, S(1.0), zero}, ez = {zero, zero, S(1.0)};
        const V3<S> jk = b2w(rot<0>(ca, sa, rot<2>(S(cps), S(sps), rot<1>(ch, sh, cross(ey, rot<1>(ck, sk, V3<S>{zero, zero, S(-0.195)}))))));     // knee axis y (H axes) x arm from the knee
        const V3<S> jh = b2w(rot<0>(ca, sa, cross(rot<2>(S(cps), S(sps), ey), dH)));                                                              // hip axis: Rz(psi) e_y in A axes
        const V3<S> ja = b2w(cross(ex, dA));                                                                                                       // abad axis x of the trunk
        Ja.r[0] = {ja.x, jh.x, jk.x}; Ja.r[1] = {ja.y, jh.y, jk.y}; Ja.r[2] = {ja.z, jh.z, jk.z};
        const V3<S> rW = b2w(rB);
        const V3<S> a3 = ez, a4 = rot<2>(T.c3, T.s3, ey), a5 = rot<2>(T.c3, T.s3, rot<1>(T.c4, T.s4, ex));
        const V3<S> j3 = cross(a3, rW), j4 = cross(a4, rW), j5 = cross(a5, rW);
        Jb[0][0] = S(1.0); Jb[0][1] = zero; Jb[0][2] = zero; Jb[1][0] = zero; Jb[1][1] = S(1.0); Jb[1][2] = zero; Jb[2][0] = zero; Jb[2][1] = zero; Jb[2][2] = S(1.0);
        Jb[0][3] = j3.x; Jb[1][3] = j3.y; Jb[2][3] = j3.z; Jb[0][4] = j4.x; Jb[1][4] = j4.y; Jb[2][4] = j4.z; Jb[0][5] = j5.x; Jb[1][5] = j5.y; Jb[2][5] = j5.z;
    }
    // (hsddp_friction.h) the lane's flag of the x and y force directions - cl for a sticking foot, 0 for a sliding one; c_z stays cl - and the known
    // tangential force of a sliding foot through J^T: ftl the lane's three leg rows, ftb the six base rows summed over the quad
    constexpr bool FRIC = (wbs_is_fric_io<LO>::value || ...);
    WbsFricIO<S>* const fio = wbs_fric_ptr<S>(lam_out...);      // (null without friction, and then never used)
    if constexpr (FRIC) wbs_fric_force<Q, S>(fio, fvel, m0);
    auto cxy_of = [&]() { return cl * (S(1.0) - wbs_fric_slot(fio, FRIC_EFF)); };      // (friction only) read from the column at every use
    // ---- contact solve, block form.  L = [ blockdiag(L_l) 0 ; E  L_S ],  E_l = Ct L_l^-T (6 x 3),  S = B - sum_l E_l E_l^T
    const Chol3<S> Ll = chol3<Q, S>(d_aa, d_ha, d_hh, d_ka, d_kh, d_kk);
    S E[6][3];
    _Pragma("unroll")
    for (int c = 0; c < 6; c++) {      // row c of E: E L^T = Ct  ->  forward substitution along the row
        E[c][0] = Ct[c][0] * Ll.r0; E[c][1] = (Ct[c][1] - E[c][0] * Ll.l10) * Ll.r1; E[c][2] = (Ct[c][2] - E[c][0] * Ll.l20 - E[c][1] * Ll.l21) * Ll.r2;
    }
    S LS[21], rdS[6];
    _Pragma("unroll")
    for (int i = 0; i < 6; i++) _Pragma("unroll") for (int j = 0; j <= i; j++) LS[tri(i, j)] = Bm[tri(i, j)] - Q::sum(E[i][0] * E[j][0] + E[i][1] * E[j][1] + E[i][2] * E[j][2]);
    chol6<Q, S>(LS, rdS);
    // y = L^-1 (tau - h): leg part in the lane, base part replicated (mode 1: no bias, y = 0)
    V3<S> yl_; S ftb[6];
    if constexpr (FRIC) {
        const S fx = wbs_fric_slot(fio, FRIC_FX), fy = wbs_fric_slot(fio, FRIC_FY);
        _Pragma("unroll") for (int c = 0; c < 6; c++) ftb[c] = Q::sum(Jb[0][c] * fx + Jb[1][c] * fy);
        yl_ = fwd3(Ll, V3<S>{m0 * (ul[0] - hl[0]) + (Ja.r[0].x * fx + Ja.r[1].x * fy), m0 * (ul[1] - hl[1]) + (Ja.r[0].y * fx + Ja.r[1].y * fy), m0 * (ul[2] - hl[2]) + (Ja.r[0].z * fx + Ja.r[1].z * fy)});
    } else yl_ = fwd3(Ll, V3<S>{m0 * (ul[0] - hl[0]), m0 * (ul[1] - hl[1]), m0 * (ul[2] - hl[2])});
    const V3<S> yl = yl_;
    S yb[6];
    if constexpr (FRIC) { _Pragma("unroll") for (int c = 0; c < 6; c++) yb[c] = (ftb[c] - m0 * hb[c]) - Q::sum(E[c][0] * yl.x + E[c][1] * yl.y + E[c][2] * yl.z); }
    else
    _Pragma("unroll") for (int c = 0; c < 6; c++) yb[c] = -(m0 * hb[c]) - Q::sum(E[c][0] * yl.x + E[c][1] * yl.y + E[c][2] * yl.z);
    fwd6(LS, rdS, yb);
    // X = L^-1 Jc^T for the lane's foot (zero for a swing leg): Xt (3 leg rows x 3 force directions), Xb (6 base rows x 3)
    M33<S> Xt; S Xb[6][3];      // Xt.r[d] = column d (force direction d) as a 3-vector over the leg rows ; Xb[c][d]
    _Pragma("unroll")
    for (int d = 0; d < 3; d++) {
        S cd = cl;      // the lane's flag of force direction d
        if constexpr (FRIC) { if (d < 2) cd = cxy_of(); }
        const V3<S> xt = scale(cd, fwd3(Ll, Ja.r[d]));      // L_l^-1 (row d of Ja)^T
        Xt.r[d] = xt;
        S w[6];
        _Pragma("unroll") for (int c = 0; c < 6; c++) w[c] = cd * Jb[d][c] - (E[c][0] * xt.x + E[c][1] * xt.y + E[c][2] * xt.z);
        fwd6(LS, rdS, w);
        _Pragma("unroll") for (int c = 0; c < 6; c++) Xb[c][d] = w[c];
    }
    // Gram matrix G = X^T X in 3 x 3 blocks: lane f holds block row f (blocks g <= f), a swing leg's diagonal block is the identity
    // (its multiplier is zero); right-hand side  -X^T y - gam,  gam = Jdot v + 2 alpha J v (WBM.cpp:392-408)
    M33<S> G[4];
    auto xb_of = [&](auto JT, int c, int d) { constexpr int J = decltype(JT)::value; return Q::template get<J>(Xb[c][d]); };
    using J0 = IC<0>; using J1 = IC<1>; using J2 = IC<2>; using J3 = IC<3>;
    auto gram_block = [&](auto JT, M33<S>& Gb) {
        S o[6][3];
        _Pragma("unroll") for (int c = 0; c < 6; c++) _Pragma("unroll") for (int d = 0; d < 3; d++) o[c][d] = xb_of(JT, c, d);
        _Pragma("unroll")
        for (int r = 0; r < 3; r++) {
            S e[3];
            _Pragma("unroll") for (int d = 0; d < 3; d++) { S s = Xb[0][r] * o[0][d]; _Pragma("unroll") for (int c = 1; c < 6; c++) s = s + Xb[c][r] * o[c][d]; e[d] = s; }
            Gb.r[r] = {e[0], e[1], e[2]};
        }
    };
    gram_block(J0{}, G[0]); gram_block(J1{}, G[1]); gram_block(J2{}, G[2]); gram_block(J3{}, G[3]);
    // the lane's own diagonal block: + Xt^T Xt + damping (contact) / identity (swing)
    M33<S> Gd;
    {
        const S dg = 1.0 - cl;      // (the damping enters at the factorisation)
        S dgx = dg;                 // (friction) a masked direction gets the identity too
        if constexpr (FRIC) dgx = 1.0 - cxy_of();
        _Pragma("unroll")
        for (int r = 0; r < 3; r++) {
            const S e0 = dot3(Xt.r[r], Xt.r[0]), e1 = dot3(Xt.r[r], Xt.r[1]), e2 = dot3(Xt.r[r], Xt.r[2]);
            Gd.r[r] = {e0 + (r == 0 ? dgx : zero), e1 + (r == 1 ? dgx : zero), e2 + (r == 2 ? dg : zero)};
        }
        // added to G[own lane]: by selects on the lane's leg
        const S m0 = Q::legc(1, 0, 0, 0), m1 = Q::legc(0, 1, 0, 0), m2 = Q::legc(0, 0, 1, 0), m3 = Q::legc(0, 0, 0, 1);
        _Pragma("unroll")
        for (int r = 0; r < 3; r++) {
            G[0].r[r] = G[0].r[r] + scale(m0, Gd.r[r]); G[1].r[r] = G[1].r[r] + scale(m1, Gd.r[r]);
            G[2].r[r] = G[2].r[r] + scale(m2, Gd.r[r]); G[3].r[r] = G[3].r[r] + scale(m3, Gd.r[r]);
        }
    }
    V3<S> rhs;
    {
        S xy[3];
        _Pragma("unroll") for (int d = 0; d < 3; d++) { S s = dot3(Xt.r[d], yl); _Pragma("unroll") for (int c = 0; c < 6; c++) s = s + Xb[c][d] * yb[c]; xy[d] = s; }
        // mode 0: gam = Jdot v + 2 alpha J v (WBM.cpp:392-408) ; mode 1: the right-hand side is -Jc v, and J v of a foot is its velocity
        const double a2 = 2.0 * bg_alpha;
        const V3<S> gam = {m0 * (jdv.x + a2 * fvel.x) + m1 * fvel.x, m0 * (jdv.y + a2 * fvel.y) + m1 * fvel.y, m0 * (jdv.z + a2 * fvel.z) + m1 * fvel.z};
        if constexpr (FRIC) { const S cxy = cxy_of(); rhs = {cxy * (-xy[0] - gam.x), cxy * (-xy[1] - gam.y), cl * (-xy[2] - gam.z)}; }
        else
        rhs = {cl * (-xy[0] - gam.x), cl * (-xy[1] - gam.y), cl * (-xy[2] - gam.z)};
    }
    // block Cholesky of G over the quad: block column kc is finished by lane kc (its diagonal block), then lanes f > kc form L_f,kc.
    // Lane f keeps its block row Lg[0..f]; blocks right of the diagonal are never used.
    M33<S> Lg[4]; Chol3<S> Ld;      // Lg[g]: block (own lane, g) of the factor, g < own lane ; Ld: the own diagonal block's factor
    {
        const S lane = Q::legc(0, 1, 2, 3);
        auto bcast33 = [&](auto JT, const M33<S>& A) { constexpr int J = decltype(JT)::value; M33<S> o; _Pragma("unroll") for (int r = 0; r < 3; r++) o.r[r] = {Q::template get<J>(A.r[r].x), Q::template get<J>(A.r[r].y), Q::template get<J>(A.r[r].z)}; return o; };
        auto bcastL = [&](auto JT, const Chol3<S>& A) { constexpr int J = decltype(JT)::value; Chol3<S> o; o.l10 = Q::template get<J>(A.l10); o.l20 = Q::template get<J>(A.l20); o.l21 = Q::template get<J>(A.l21); o.r0 = Q::template get<J>(A.r0); o.r1 = Q::template get<J>(A.r1); o.r2 = Q::template get<J>(A.r2); return o; };
        // A <- A - P Q^T (3x3 blocks, rows)
        auto sub_abt = [&](M33<S>& A, const M33<S>& Pm, const M33<S>& Qm) { _Pragma("unroll") for (int r = 0; r < 3; r++) A.r[r] = A.r[r] - V3<S>{dot3(Pm.r[r], Qm.r[0]), dot3(Pm.r[r], Qm.r[1]), dot3(Pm.r[r], Qm.r[2])}; };
        // rows of A <- (rows of A) L^-T : solve x L^T = a per row
        auto right_solve = [&](M33<S>& A, const Chol3<S>& Lk) { _Pragma("unroll") for (int r = 0; r < 3; r++) { V3<S> a = A.r[r], x; x.x = a.x * Lk.r0; x.y = (a.y - x.x * Lk.l10) * Lk.r1; x.z = (a.z - x.x * Lk.l20 - x.y * Lk.l21) * Lk.r2; A.r[r] = x; } };
        // own diagonal block = G[own]: picked by selects (each lane needs ITS block at ITS step; every lane runs every step)
        const S dmp = cl * damping;
        S dmpx = dmp;      // (friction) the damping goes to constrained directions only
        if constexpr (FRIC) dmpx = cxy_of() * damping;
        auto own_diag = [&](const M33<S>& Gk) { return chol3<Q, S>(Gk.r[0].x + dmpx, Gk.r[1].x, Gk.r[1].y + dmpx, Gk.r[2].x, Gk.r[2].y, Gk.r[2].z + dmp); };
        // step 0: lane 0's diagonal block is final
        Chol3<S> L0 = own_diag(G[0]);                       // meaningful in lane 0
        const Chol3<S> L00 = bcastL(J0{}, L0);
        Lg[0] = G[0]; right_solve(Lg[0], L00);              // lanes 1..3: L_f0 (lane 0's own copy is not used)
        // step 1
        const M33<S> L10 = bcast33(J1{}, Lg[0]);
        M33<S> A1 = G[1]; sub_abt(A1, Lg[0], L10);          // lanes >= 1: G_f1 - L_f0 L_10^T
        Chol3<S> L1 = own_diag(A1);                         // meaningful in lane 1
        const Chol3<S> L11 = bcastL(J1{}, L1);
        Lg[1] = A1; right_solve(Lg[1], L11);                // lanes 2..3: L_f1
        // step 2
        const M33<S> L20 = bcast33(J2{}, Lg[0]), L21 = bcast33(J2{}, Lg[1]);
        M33<S> A2 = G[2]; sub_abt(A2, Lg[0], L20); sub_abt(A2, Lg[1], L21);
        Chol3<S> L2 = own_diag(A2);                         // meaningful in lane 2
        const Chol3<S> L22 = bcastL(J2{}, L2);
        Lg[2] = A2; right_solve(Lg[2], L22);                // lane 3: L_32
        // step 3
        M33<S> A3 = G[3]; sub_abt(A3, Lg[0], Lg[0]); sub_abt(A3, Lg[1], Lg[1]); sub_abt(A3, Lg[2], Lg[2]);      // lane 3: G_33 - sum L_3g L_3g^T
        Chol3<S> L3 = own_diag(A3);                         // meaningful in lane 3
        // every lane keeps its own diagonal factor
        const typename Q::B is0 = Q::gt(S(0.5), lane), is1 = Q::gt(S(1.5), lane), is2 = Q::gt(S(2.5), lane);
        auto pick = [&](const S& a0, const S& a1, const S& a2, const S& a3) { return Q::sel(is0, a0, Q::sel(is1, a1, Q::sel(is2, a2, a3))); };
        Ld.l10 = pick(L0.l10, L1.l10, L2.l10, L3.l10); Ld.l20 = pick(L0.l20, L1.l20, L2.l20, L3.l20); Ld.l21 = pick(L0.l21, L1.l21, L2.l21, L3.l21);
        Ld.r0 = pick(L0.r0, L1.r0, L2.r0, L3.r0); Ld.r1 = pick(L0.r1, L1.r1, L2.r1, L3.r1); Ld.r2 = pick(L0.r2, L1.r2, L2.r2, L3.r2);
        // lam = G^-1 rhs: forward over block rows 0..3, backward 3..0.  z_f lives in lane f.
        V3<S> z = rhs;
        auto bc3 = [&](auto JT, const V3<S>& w) { constexpr int J = decltype(JT)::value; return V3<S>{Q::template get<J>(w.x), Q::template get<J>(w.y), Q::template get<J>(w.z)}; };
        V3<S> z0 = fwd3(Ld, z);                                               // valid in lane 0
        const V3<S> Z0 = bc3(J0{}, z0);
        V3<S> t1 = z - m33_mul(Lg[0], Z0); V3<S> z1 = fwd3(Ld, t1);            // valid in lane 1
        const V3<S> Z1 = bc3(J1{}, z1);
        V3<S> t2 = t1 - m33_mul(Lg[1], Z1); V3<S> z2 = fwd3(Ld, t2);           // valid in lane 2
        const V3<S> Z2 = bc3(J2{}, z2);
        V3<S> t3 = t2 - m33_mul(Lg[2], Z2); V3<S> z3 = fwd3(Ld, t3);           // valid in lane 3
        z = {pick(z0.x, z1.x, z2.x, z3.x), pick(z0.y, z1.y, z2.y, z3.y), pick(z0.z, z1.z, z2.z, z3.z)};
        // backward: lam_3 = L_33^-T z_3 ; lam_k = L_kk^-T (z_k - sum_{f>k} L_fk^T lam_f) - the product L_fk^T lam_f is formed in lane f and read by lane k
        V3<S> lam3 = bwd3(Ld, z);                                             // valid in lane 3
        const V3<S> w32 = bc3(J3{}, m33_mulT(Lg[2], lam3)), w31 = bc3(J3{}, m33_mulT(Lg[1], lam3)), w30 = bc3(J3{}, m33_mulT(Lg[0], lam3));
        V3<S> lam2 = bwd3(Ld, z - w32);                                       // valid in lane 2
        const V3<S> w21 = bc3(J2{}, m33_mulT(Lg[1], lam2)), w20 = bc3(J2{}, m33_mulT(Lg[0], lam2));
        V3<S> lam1 = bwd3(Ld, z - w31 - w21);                                 // valid in lane 1
        const V3<S> w10 = bc3(J1{}, m33_mulT(Lg[0], lam1));
        V3<S> lam0 = bwd3(Ld, z - w30 - w20 - w10);                           // valid in lane 0
        rhs = {pick(lam0.x, lam1.x, lam2.x, lam3.x), pick(lam0.y, lam1.y, lam2.y, lam3.y), pick(lam0.z, lam1.z, lam2.z, lam3.z)};
    }
    V3<S> lam_;
    if constexpr (FRIC) { const S cxy = cxy_of(); lam_ = {cxy * rhs.x, cxy * rhs.y, cl * rhs.z}; }      // (a sliding foot's tangential multipliers are zero: its force there is f_t)
    else lam_ = scale(cl, rhs);
    const V3<S> lam = lam_;      // contact force of the lane's foot (world axes); zero for a swing leg
    if constexpr (PLANT || FRIC || (wbs_is_ter_io<LO>::value || ...)) { ((lam_out->lam = lam, lam_out->pz = fpos.z, lam_out->wz = fvel.z, lam_out->px = fpos.x, lam_out->py = fpos.y), ...); }
    else if constexpr ((wbs_is_uni_io<LO>::value || ...)) { ((lam_out->lam = lam, lam_out->pz = fpos.z, lam_out->wz = fvel.z), ...); }
    else if constexpr (sizeof...(LO) > 0) { ((lam_out != nullptr ? (void)(*lam_out = lam) : (void)0), ...); }
    // qdd = L^-T (y + X lam): base part replicated, leg part in the lane
    S qddb[6]; V3<S> qddl;
    {
        _Pragma("unroll") for (int c = 0; c < 6; c++) qddb[c] = yb[c] + Q::sum(Xb[c][0] * lam.x + Xb[c][1] * lam.y + Xb[c][2] * lam.z);
        bwd6(LS, rdS, qddb);
        V3<S> zl = yl + V3<S>{Xt.r[0].x * lam.x + Xt.r[1].x * lam.y + Xt.r[2].x * lam.z, Xt.r[0].y * lam.x + Xt.r[1].y * lam.y + Xt.r[2].y * lam.z, Xt.r[0].z * lam.x + Xt.r[1].z * lam.y + Xt.r[2].z * lam.z};
        S et[3];
        _Pragma("unroll") for (int j = 0; j < 3; j++) { S s = E[0][j] * qddb[0]; _Pragma("unroll") for (int c = 1; c < 6; c++) s = s + E[c][j] * qddb[c]; et[j] = s; }
        qddl = bwd3(Ll, zl - V3<S>{et[0], et[1], et[2]});
    }
    // mode 1: the velocities after the impact, v + L^-T X lam
    _Pragma("unroll") for (int c = 0; c < 6; c++) out_b[c] = qddb[c] + m1 * vb[c];
    out_l = {qddl.x + m1 * vl_[0], qddl.y + m1 * vl_[1], qddl.z + m1 * vl_[2]};
}

// per-sample summary of a window, as the kernel leaves it (doubles; hsddp_sim_get_rows turns first_bad into an int)
constexpr int SIM_PARK = 24;     // doubles a lane parks in LDS across the contact solve (wbs_walk)
constexpr int SIM_ROW = 5;      // dev_q | dev_v | min_height | max_torque | first_bad

// The window of one (problem b, sample) pair, quad index g = b * R + sample, walked by a lane quad.
//   map: [3][n_steps] step -> phase, knot of the phase, 1 if the phase's reset map is applied behind the step (last knot of a phase with a touchdown,
//        and the window goes on), as hsddp_sim_create lays it out
//   x0: [B R][36]; xfinal: [B R][36]; rows: [B R][SIM_ROW]; trajX: [B R][n_steps + 1][36] or null; trajU: [B R][n_steps][12] or null
//   stash: SIM_PARK x 64 doubles of LDS of the wave (device only)
// A quad whose new state fails the rollout's divergence test (squared norm above 1e12 or NaN, wb_quad.hpp / SinglePhase.cpp:205) keeps the state it
// had BEFORE that step and records nothing further, but goes on executing: the cross-lane steps need all four lanes, and the other quads of the
// wave must not notice.  Trajectory entries behind first_bad repeat the kept state (controls: what the policy asks for there).
//
// Disturbances (include/hsddp_mc.h): the policy D, empty for the plain walk.  WbsMc points at the switches of a disturbed run; every `if constexpr
// (D::MC)` below is its code, and with WbsPlain none of it exists: k_sim_quad compiles to what it compiled to before the policy was there.
struct WbsMcArgs {
    unsigned long long seed, first_problem;      // the generator's key; global index of problem 0 of the handle
    double su, sq, sv, umax, fall;              // sigma_u, sigma_q, sigma_v (0: off), u_max, fall_height (<= 0: off)
    int kick_step, R;                           // step of the push (-1: none); samples per problem
    const double* kick; double* extra;          // [B R][36] or null; [B R][2] first_fall | n_sat
};
// NOISE 0: the walk of a run whose three sigmas are zero, compiled without the generator.  Measured (MI355X, config 3 x 16 samples x 200 steps, plain
// run 9.88 ms): with the generator compiled in and branched over, a run with only u_max set took 11.74 ms - the register allocation of the whole
// loop pays for code that does not run; without it 9.83 ms.  So the host picks the instantiation, and every other switch stays a run-time branch.
struct WbsPlain { static constexpr int MC = 0, NOISE = 0, GRF = 0, SUB = 0, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; };
template <int NOISE_> struct WbsMc { static constexpr int MC = 1, NOISE = NOISE_, GRF = 0, SUB = 0, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsMcArgs* a; };
constexpr int SIM_PARK_MC = SIM_PARK + 2;       // ... and n_sat, first_fall
// Contact-force records (include/hsddp_grf.h): GRF 1 in the policy.  The walk takes the lane's multiplier of every mode-0 solve, keeps five running
// values per lane (lane = leg) - smallest / largest stance fz, smallest cone margin, first violating step, violations - and joins them over the
// quad at the end; every `if constexpr (D::GRF)` below is its code, and the policies above compile to what they compiled to without it.  The
// thresholds and the destinations live in device memory and are read through a laundered pointer, as the switches of a disturbed run are.
struct WbsGrfArgs {
    double mu, fz_min;          // friction coefficient of the pyramid (> 0); smallest admissible normal force
    double* rows; double* Y;    // [B R][SIM_GRF_ROW]; [B R][n_steps][12] or null
};
constexpr int SIM_GRF_ROW = 5;     // min_fz | min_cone | max_fz | first_slip | n_slip
constexpr int SIM_GRF_PARK = 5;    // the lane's running values, parked behind the others
constexpr double SIM_GRF_NONE = 1e18;      // first_slip of a lane without a violation while the walk runs: above every step index
struct WbsGrf { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 0, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsGrfArgs* gr; };
template <int NOISE_> struct WbsMcGrf { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 0, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; };
// Sub-stepped integration (include/hsddp_substep.h): SUB 1 in the policy.  A control knot is S forward-Euler steps of dt / S under the knot's torque
// (zero-order hold): the feedback, the noise and every record of the state stay once per control step, the contact solve, the divergence test and
// the force records run once per substep.  S is a run-time trip count read from device memory through a laundered pointer, as the other switches
// are.  The lane's three torques now live across contact solves and join the parked column (SIM_SUB_PARK, behind everything else); every `if
// constexpr (D::SUB)` below is this code, and the six policies above compile to what they compiled to without it.
struct WbsSubArgs { int substeps, pad; };      // 2 .. 64 (the host launches the kernels above for 1)
constexpr int SIM_SUB_PARK = 3;
struct WbsSub { static constexpr int MC = 0, NOISE = 0, GRF = 0, SUB = 1, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsSubArgs* sb; };
template <int NOISE_> struct WbsMcSub { static constexpr int MC = 1, NOISE = NOISE_, GRF = 0, SUB = 1, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsMcArgs* a; const WbsSubArgs* sb; };
struct WbsGrfSub { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; };
template <int NOISE_> struct WbsMcGrfSub { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 0, TER = 0, PLANT = 0, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; };
// Unilateral ground contact (include/hsddp_contact.h): UNI 1 in the policy, always with the records and the sub-step loop (GRF 1, SUB 1; S = 1 too).
// The lane (= leg) carries F, 1 if its foot is a scheduled stance foot that is FREE, and the contact flag of every solve is the lane's own: attached =
// scheduled and not free.  The trip loop of a control step becomes a small state machine around the ONE call site of the solve -
//     substep:  solve -> [landing impact on T, solve] -> [release the foot that pulls hardest, solve]* -> records, Euler step
// - that advances on wave-uniform decisions (a ballot over the wave): a trip is repeated if ANY quad of the wave needs it, and a quad that does not
// repeats the solve with its own unchanged set and state, which gives it the same numbers (the impact trip is not applied to it: a select).  F, the
// landing set T, the four counters and max_lift are parked with the rest.  Every `if constexpr (D::UNI)` below is this code, and the twelve policies
// above compile to what they compiled to without it.
struct WbsUniArgs {
    double fz_rel, z_ground;      // a foot whose normal force falls below fz_rel is released; height of the flat ground, world z
    double* rows;                 // [B R][SIM_UNI_ROW]
    double* F;                    // [B R][4] the free flags carried from run to run (episodes), loaded at the head and stored at the end; null: F starts empty
    const int* hold; int hold_stride, pad;      // (episodes) hold[g hold_stride] != 0: sample g is frozen and keeps the F it had; null: every sample stores
};
constexpr int SIM_UNI_ROW = 6;      // first_release | n_release | n_land | n_free | free_final | max_lift
constexpr int SIM_UNI_PARK = 7;     // F, T, first_release, n_release, n_land, n_free, max_lift of the lane, parked behind everything else
struct WbsUni { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 1, TER = 0, PLANT = 0, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; };
template <int NOISE_> struct WbsMcUni { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 1, TER = 0, PLANT = 0, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; };
// Terrain and early swing-foot touchdown (include/hsddp_terrain.h): TER 1 in the policy, on top of UNI = GRF = SUB = 1.  The landing test compares with
// a looked-up height instead of a constant, the tested set grows by the swing feet, and the attached set of a solve by the swing feet that landed: the
// lane carries E, 1 if its foot is a SWING foot that is attached.  The solve hands the foot's x and y back through WbsTerIO; the lookup is one per-lane
// load behind the solve of stage 0.  E, the four counters and max_pen are parked behind everything else.  Every `if constexpr (D::TER)` below is this
// code, and the fifteen policies above compile to what they compiled to without it.
struct WbsTerArgs {
    const double* H;              // [n_maps][ny][nx]
    const int* map_of;            // [B R] the map of a sample
    int nx, ny, n_maps, early;
    double x0, y0, cx, cy, w_td;
    double* rows;                 // [B R][SIM_TER_ROW]
    double* E;                    // [B R][4] the early flags carried from run to run (episodes), as WbsUniArgs::F (and under its hold); null: E starts empty
};
constexpr int SIM_TER_ROW = 6;      // first_early | n_early | n_early_release | n_held | early_final | max_pen
constexpr int SIM_TER_PARK = 6;     // E, first_early, n_early, n_early_release, n_held, max_pen of the lane
struct WbsTer { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 0, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; };
template <int NOISE_> struct WbsMcTer { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 0, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; };
template <bool TER, class S> struct wbs_io_of { using type = WbsUniIO<S>; };
template <class S> struct wbs_io_of<true, S> { using type = WbsTerIO<S>; };
// Plant-model mismatch (include/hsddp_plant.h): PLANT 1 in the policy, always with the records and the sub-step loop (GRF 1, SUB 1; S = 1 too), on top of
// any of the three families - the bilateral walk, the unilateral one, the one with terrain.  The quad reads its row of the table through plant_of[g] in
// front of every solve: the solve takes the inertias from it (WbsPlantIO), and the torque it is given is  gain o u - damping o qdot_leg  of the state that
// solve starts from, formed from six per-lane loads at the call.  ul stays the commanded torque: it is what U, max_torque and n_sat record and what is
// parked.  Nothing of the row is carried across a solve.  Every `if constexpr (D::PLANT)` below is this code, and the policies above compile to what
// they compiled to without it.
constexpr int SIM_PLANT_ROW = 46;      // HSDDP_PLANT_ROW: trunk mass | CoM 3 | inertia 6 | link_scale 12 | tau_gain 12 | damping 12
struct WbsPlantArgs {
    const double* P;              // [n_plants][SIM_PLANT_ROW]
    const int* plant_of;          // [B R] the row of a sample, checked against n_plants by the host
    int n_plants, pad;
};
struct WbsPlant { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 0, TER = 0, PLANT = 1, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsPlantArgs* pl; };
template <int NOISE_> struct WbsMcPlant { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 0, TER = 0, PLANT = 1, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsPlantArgs* pl; };
struct WbsUniPlant { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 1, TER = 0, PLANT = 1, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsPlantArgs* pl; };
template <int NOISE_> struct WbsMcUniPlant { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 1, TER = 0, PLANT = 1, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsPlantArgs* pl; };
struct WbsTerPlant { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 1, FRIC = 0; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; const WbsPlantArgs* pl; };
template <int NOISE_> struct WbsMcTerPlant { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 1, FRIC = 0; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; const WbsPlantArgs* pl; };
template <bool PLANT, bool TER, class S> struct wbs_io_sel { using type = typename wbs_io_of<TER, S>::type; };
template <bool TER, class S> struct wbs_io_sel<true, TER, S> { using type = WbsPlantIO<S>; };
// Coulomb friction (include/hsddp_friction.h): FRIC 1 in the policy, on top of UNI = TER = GRF = SUB = 1 (with the terrain off the host binds a one-cell
// flat map with early = 0, which is the contact rule alone).  The lane carries the sliding flag of its foot, the fresh flag, the lagged normal force and
// the direction of a fresh foot's friction; every mode-0 solve takes them through WbsFricIO and treats a sliding foot with its z row alone.  Behind the
// lift-off test of a solve comes the onset test - the sticking attached foot with the smallest circular-cone margin mu_s lambda_z - |lambda_t| joins the
// sliding set if that margin is negative - as one more reason to solve again.  The flags, n_f, the direction and the six running values of the row are
// parked behind everything else.  Every `if constexpr (D::FRIC)` below is this code, and the policies above compile to what they compiled to without it.
struct WbsFricArgs {
    const double* mu;             // [n_mu][2] mu_s | mu_k
    const int* mu_of;             // [B R] the row of a sample, checked against n_mu by the host
    int n_mu, pad;
    double v_stick;               // a sliding foot slower than this re-sticks
    double* rows;                 // [B R][SIM_FRIC_ROW]
    double *Sl, *NF;              // [B R][4] twice: the sliding flags and lagged normal forces carried from run to run (episodes), as WbsUniArgs::F (and under its hold); null: Sl starts empty
};
constexpr int SIM_FRIC_ROW = 7;      // first_slide | n_onset | n_slide | n_restick | slide_final | max_speed | distance
constexpr int SIM_FRIC_PARK = FRIC_SLOTS;    // sl, fresh, n_f, t_x, t_y, first_slide, n_onset, n_slide, n_restick, max_speed, distance of the lane, and the five slots the solve writes (WbsFricIO)
struct WbsFric { static constexpr int MC = 0, NOISE = 0, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 0, FRIC = 1; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; const WbsFricArgs* fc; };
template <int NOISE_> struct WbsMcFric { static constexpr int MC = 1, NOISE = NOISE_, GRF = 1, SUB = 1, UNI = 1, TER = 1, PLANT = 0, FRIC = 1; const WbsMcArgs* a; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; const WbsFricArgs* fc; };
template <bool FRIC, bool PLANT, bool TER, class S> struct wbs_io_pick { using type = typename wbs_io_sel<PLANT, TER, S>::type; };
template <bool PLANT, bool TER, class S> struct wbs_io_pick<true, PLANT, TER, S> { using type = WbsFricIO<S>; };
// Height of map m at the foot point (px, py), relative to z_ground (sim.terrain_height is the definition).  The cell index is clamped as a double - fmax
// sends a NaN to 0, fmin an infinity to the last cell - BEFORE it becomes an integer: no address outside the grid can be formed, whatever the state holds.
HD double wbs_ter_height_lane(const WbsTerArgs& t, int m, double px, double py) {
    const double fx = fmin(fmax(floor((px - t.x0) / t.cx), 0.0), (double)(t.nx - 1));
    const double fy = fmin(fmax(floor((py - t.y0) / t.cy), 0.0), (double)(t.ny - 1));
    return t.H[((size_t)m * (size_t)t.ny + (size_t)(int)fy) * (size_t)t.nx + (size_t)(int)fx];
}

// The generator (sim.mc_normals is its definition): draw(n) is output n >= 1 of SplitMix64(seed), whose state is the counter seed + n G; the normal of
// coordinate c of (global problem, sample, step) is Box-Muller on draws n0 + 1 and n0 + 2, n0 = 2 (((problem 65536 + sample) 65536 + step) 48 + c).
constexpr unsigned long long WBS_MC_G = 0x9E3779B97F4A7C15ull;
HD double wbs_mc_unit(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
HD double wbs_mc_draw(unsigned long long seed, unsigned long long n) { return wbs_mc_unit(seed + n * WBS_MC_G); }
// three normals per lane: coordinates c, c + 1, c + 2 of the (problem, sample, step) numbered `base`; c is the lane's own (a small integer in a double)
HD void wbs_mc_normal3_lane(unsigned long long seed, unsigned long long base, int c, double (&z)[3]) {
    unsigned long long st = seed + (2ull * (base * 48ull + (unsigned long long)c)) * WBS_MC_G;
    _Pragma("unroll")
    for (int j = 0; j < 3; j++) {
        const double u1 = wbs_mc_unit(st + WBS_MC_G), u2 = wbs_mc_unit(st + 2ull * WBS_MC_G);
        st += 2ull * WBS_MC_G;
        // (1 - u1 is in (0, 1].)  On the device cos(2 pi u2) is cospi(2 u2) of the device library: the same number without the rounding of 2 pi u2 and
        // without cos's argument reduction - 19.9 -> 18.3 ms with all three sigmas on (same measurement as above)
#ifdef HS_HOST_EMU
        z[j] = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
#else
        z[j] = sqrt(-2.0 * log(1.0 - u1)) * cospi(2.0 * u2);
#endif
    }
}
#ifdef HS_HOST_EMU
inline void wbs_mc_normal3(unsigned long long seed, unsigned long long base, const Q4& c, Q4 (&z)[3]) {
    for (int l = 0; l < 4; l++) { double t[3]; wbs_mc_normal3_lane(seed, base, (int)c.v[l], t); for (int j = 0; j < 3; j++) z[j].v[l] = t[j]; }
}
inline const WbsMcArgs* wbs_mc_fresh(const WbsMcArgs* p) { return p; }
inline const WbsGrfArgs* wbs_grf_fresh(const WbsGrfArgs* p) { return p; }
inline const WbsSubArgs* wbs_sub_fresh(const WbsSubArgs* p) { return p; }
inline const WbsUniArgs* wbs_uni_fresh(const WbsUniArgs* p) { return p; }
inline const WbsTerArgs* wbs_ter_fresh(const WbsTerArgs* p) { return p; }
inline const WbsPlantArgs* wbs_plant_fresh(const WbsPlantArgs* p) { return p; }
inline const WbsFricArgs* wbs_fric_fresh(const WbsFricArgs* p) { return p; }
inline Q4 wbs_ter_height(const WbsTerArgs& t, int m, const Q4& px, const Q4& py) { return Q4(wbs_ter_height_lane(t, m, px.v[0], py.v[0]), wbs_ter_height_lane(t, m, px.v[1], py.v[1]), wbs_ter_height_lane(t, m, px.v[2], py.v[2]), wbs_ter_height_lane(t, m, px.v[3], py.v[3])); }
inline bool wbs_any(const Q4& f) { return f.v[0] > 0.5 || f.v[1] > 0.5 || f.v[2] > 0.5 || f.v[3] > 0.5; }      // (host: the quad is the whole wave)
#else
HD void wbs_mc_normal3(unsigned long long seed, unsigned long long base, const double& c, double (&z)[3]) { wbs_mc_normal3_lane(seed, base, (int)c, z); }
// the switches are read again at every step from a pointer the compiler cannot see through: held in scalar registers across the contact solve
// they were spilled (as kernel arguments by value: 94 scalar registers in scratch)
HD const WbsMcArgs* wbs_mc_fresh(const WbsMcArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsGrfArgs* wbs_grf_fresh(const WbsGrfArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsSubArgs* wbs_sub_fresh(const WbsSubArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsUniArgs* wbs_uni_fresh(const WbsUniArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsTerArgs* wbs_ter_fresh(const WbsTerArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsPlantArgs* wbs_plant_fresh(const WbsPlantArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD const WbsFricArgs* wbs_fric_fresh(const WbsFricArgs* p) { asm volatile("" : "+s"(p)); return p; }
HD double wbs_ter_height(const WbsTerArgs& t, int m, double px, double py) { return wbs_ter_height_lane(t, m, px, py); }
// true if the 0 / 1 flag is set in ANY active lane of the wave: a ballot, so the answer is wave-uniform and the branch on it a scalar one
HD bool wbs_any(double f) { return __builtin_amdgcn_ballot_w64(f > 0.5) != 0ull; }
#endif

template <class Q, class D = WbsPlain>
HD void wbs_walk(PhaseC* ph, const ModelDev& md, const int* map, int n_steps, int b, size_t g, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU,
                 double* stash = nullptr, const D& dist = D()) {
    using S = typename Q::S;
    const S zero = S(0.0), one = S(1.0);
    const S w0 = Q::legc(1.0, 0.0, 0.0, 0.0);      // the replicated base entries are counted once
    S qb[6], vb[6], ql[3], vl[3];
    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::ld(x0, g * 36 + i, 0); vb[i] = Q::ld(x0, g * 36 + 18 + i, 0); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::ld(x0, g * 36 + 6 + j, 3); vl[j] = Q::ld(x0, g * 36 + 24 + j, 3); }
    S alive = one, first_bad = S(-1.0);
    S nsat = zero, ffall = S(-1.0);             // (disturbed walk only) saturated torques of the lane's leg; first step below fall_height
    S dq = zero, dv = zero, umax = zero, hmin = qb[2];      // (per-lane maxima over the base and the lane's leg: joined over the quad at the end)
    // (records only) of the lane's foot while it is a stance foot: smallest / largest fz, smallest cone margin, first violating step, violations
    S gfmin = S(HUGE_VAL), gcmin = S(HUGE_VAL), gfmax = S(-HUGE_VAL), gfirst = S(SIM_GRF_NONE), gslip = zero;
    // (unilateral contact only) F and the landing set T of the lane's foot, 0 / 1; first control step with a release; releases, landings and free
    // (foot, substep) pairs of the lane's foot; largest height of the foot above the ground at a landing test
    S fr = zero, tl = zero, ufirst = S(-1.0), nrel = zero, nland = zero, nfree = zero, mlift = S(-HUGE_VAL);
    if constexpr (D::UNI) { const WbsUniArgs ua = *wbs_uni_fresh(dist.un); if (ua.F != nullptr) fr = Q::ld(ua.F, g * 4, 1); }
    // (terrain only) E of the lane's foot, 0 / 1; first control step with an early touchdown (the quad's, replicated); early touchdowns, releases from E
    // and held (foot, substep) pairs of the lane's foot; largest depth of the foot below the ground at a landing
    S er = zero, efirst = S(-1.0), nearly = zero, nerel = zero, nheld = zero, mpen = S(-HUGE_VAL);
    if constexpr (D::TER) { const WbsTerArgs ta = *wbs_ter_fresh(dist.te); if (ta.E != nullptr) er = Q::ld(ta.E, g * 4, 1); }
    // (friction only) the lane's friction column (the slots of WbsFricIO): of the lane's foot - in the sliding set, 0 / 1; joined it in this substep; the
    // lagged normal force; the direction of a fresh foot's friction; first control step with an onset (the quad's, replicated); onsets, sliding (foot,
    // substep) pairs and re-sticks; largest sliding speed; path.  On the device it LIVES in the lane's column of the parked block, behind the terrain's
    // values, and every use reads or writes it there: carried in registers, its eleven doubles spilled at the feedback's register peak.
#ifdef HS_HOST_EMU
    S fcol[D::FRIC ? (int)FRIC_SLOTS : 1];
    WbsFricIO<S> fcell; fcell.col = fcol; fcell.stride = 1;
#else
    WbsFricIO<S> fcell; fcell.col = stash + threadIdx.x + 64 * ((D::MC ? SIM_PARK_MC : SIM_PARK) + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK); fcell.stride = 64;
#endif
    auto fs = [&](int i) -> S& { return wbs_fric_slot(&fcell, i); };
    if constexpr (D::FRIC) {
        const WbsFricArgs fa = *wbs_fric_fresh(dist.fc);
        _Pragma("unroll") for (int i = 0; i < FRIC_SLOTS; i++) fs(i) = zero;
        fs(FRIC_FIRST) = S(-1.0);
        if (fa.Sl != nullptr) { fs(FRIC_SL) = Q::ld(fa.Sl, g * 4, 1); fs(FRIC_NF) = Q::ld(fa.NF, g * 4, 1); }
    }
    // deviation of the state from row `kx` of a phase's Xbar: base part replicated, the lane's leg
    auto deviation = [&](PhaseC& P, size_t kx, S (&eb)[6], S (&wb)[6], S (&el)[3], S (&wl)[3]) {
        _Pragma("unroll") for (int i = 0; i < 6; i++) { eb[i] = qb[i] - Q::ld(P.Xbar, kx + i, 0); wb[i] = vb[i] - Q::ld(P.Xbar, kx + 18 + i, 0); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) { el[j] = ql[j] - Q::ld(P.Xbar, kx + 6 + j, 3); wl[j] = vl[j] - Q::ld(P.Xbar, kx + 24 + j, 3); }
    };
    auto record = [&](const S (&eb)[6], const S (&wb)[6], const S (&el)[3], const S (&wl)[3]) {
        const typename Q::B on = Q::gt(alive, S(0.5));
        S mq = zero, mv = zero;
        _Pragma("unroll") for (int i = 0; i < 6; i++) { mq = wbs_max<Q, S>(mq, wbs_abs<Q, S>(eb[i])); mv = wbs_max<Q, S>(mv, wbs_abs<Q, S>(wb[i])); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) { mq = wbs_max<Q, S>(mq, wbs_abs<Q, S>(el[j])); mv = wbs_max<Q, S>(mv, wbs_abs<Q, S>(wl[j])); }
        dq = Q::sel(on, wbs_max<Q, S>(dq, mq), dq); dv = Q::sel(on, wbs_max<Q, S>(dv, mv), dv);
        hmin = Q::sel(on, Q::min(hmin, qb[2]), hmin);
    };
    auto store_state = [&](size_t o) {
        _Pragma("unroll") for (int i = 0; i < 6; i++) { Q::st0(trajX, o + i, qb[i]); Q::st0(trajX, o + 18 + i, vb[i]); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) { Q::st(trajX, o + 6 + j, 3, ql[j]); Q::st(trajX, o + 24 + j, 3, vl[j]); }
    };
    // What the loop carries - the state (18 doubles) and the summaries (6) - is not needed while the contact solve is at its register peak, and
    // k_rollout_quad's dynamics alone take 478 of the 512 registers: the compiler spilled 76 registers to scratch to carry them.  The lane parks
    // them in a column of LDS of its own around the call instead (24 x 64 doubles = 12 KB per wave; lane-private, so no barrier): 304 -> 52 B of
    // scratch per lane, 13.6 -> 11.0 ms at config 3 x 16 samples x 200 steps.  The empty asm keeps the compiler from forwarding the registers.
#ifdef HS_HOST_EMU
    auto park = [](bool, S*) {};
#else
    auto park = [&](bool out, S* u3) {      // u3: the lane's torques, parked by the sub-stepped walk alone
        S* const c = stash + threadIdx.x;
        S* v[24] = {&qb[0], &qb[1], &qb[2], &qb[3], &qb[4], &qb[5], &vb[0], &vb[1], &vb[2], &vb[3], &vb[4], &vb[5], &ql[0], &ql[1], &ql[2], &vl[0], &vl[1], &vl[2],
                    &dq, &dv, &umax, &hmin, &alive, &first_bad};
        constexpr int G0 = D::MC ? SIM_PARK_MC : SIM_PARK;      // (records) the five running values behind the others
        constexpr int U0 = G0 + (D::GRF ? SIM_GRF_PARK : 0);    // (substeps) the torques behind those
        constexpr int N0 = U0 + (D::SUB ? SIM_SUB_PARK : 0);    // (unilateral contact) F, T, the counters and max_lift behind those
        constexpr int T0 = N0 + (D::UNI ? SIM_UNI_PARK : 0);    // (terrain) E, its counters and max_pen behind those
        // (friction: the SIM_FRIC_PARK doubles behind those are never in registers across a step, see fcell above)
        if (out) {
            _Pragma("unroll") for (int i = 0; i < 24; i++) c[64 * i] = *v[i]; if constexpr (D::MC) { c[64 * 24] = nsat; c[64 * 25] = ffall; }
            if constexpr (D::GRF) { c[64 * G0] = gfmin; c[64 * (G0 + 1)] = gcmin; c[64 * (G0 + 2)] = gfmax; c[64 * (G0 + 3)] = gfirst; c[64 * (G0 + 4)] = gslip; }
            if constexpr (D::SUB) { c[64 * U0] = u3[0]; c[64 * (U0 + 1)] = u3[1]; c[64 * (U0 + 2)] = u3[2]; }
            if constexpr (D::UNI) { c[64 * N0] = fr; c[64 * (N0 + 1)] = tl; c[64 * (N0 + 2)] = ufirst; c[64 * (N0 + 3)] = nrel; c[64 * (N0 + 4)] = nland; c[64 * (N0 + 5)] = nfree; c[64 * (N0 + 6)] = mlift; }
            if constexpr (D::TER) { c[64 * T0] = er; c[64 * (T0 + 1)] = efirst; c[64 * (T0 + 2)] = nearly; c[64 * (T0 + 3)] = nerel; c[64 * (T0 + 4)] = nheld; c[64 * (T0 + 5)] = mpen; }
        } else {
            asm volatile("" ::: "memory"); _Pragma("unroll") for (int i = 0; i < 24; i++) *v[i] = c[64 * i]; if constexpr (D::MC) { nsat = c[64 * 24]; ffall = c[64 * 25]; }
            if constexpr (D::GRF) { gfmin = c[64 * G0]; gcmin = c[64 * (G0 + 1)]; gfmax = c[64 * (G0 + 2)]; gfirst = c[64 * (G0 + 3)]; gslip = c[64 * (G0 + 4)]; }
            if constexpr (D::SUB) { u3[0] = c[64 * U0]; u3[1] = c[64 * (U0 + 1)]; u3[2] = c[64 * (U0 + 2)]; }
            if constexpr (D::UNI) { fr = c[64 * N0]; tl = c[64 * (N0 + 1)]; ufirst = c[64 * (N0 + 2)]; nrel = c[64 * (N0 + 3)]; nland = c[64 * (N0 + 4)]; nfree = c[64 * (N0 + 5)]; mlift = c[64 * (N0 + 6)]; }
            if constexpr (D::TER) { er = c[64 * T0]; efirst = c[64 * (T0 + 1)]; nearly = c[64 * (T0 + 2)]; nerel = c[64 * (T0 + 3)]; nheld = c[64 * (T0 + 4)]; mpen = c[64 * (T0 + 5)]; }
        }
    };
#endif
    // the rows of a knot the feedback reads: Xbar (base q, base v, leg q, leg v), Ubar and the lane's three rows of K
    S Xr[18], Ur[3], Kr[3][36];
    auto fetch = [&](PhaseC& P, size_t kx, size_t ku, size_t kg) {
        _Pragma("unroll") for (int i = 0; i < 6; i++) { Xr[i] = Q::ld(P.Xbar, kx + i, 0); Xr[6 + i] = Q::ld(P.Xbar, kx + 18 + i, 0); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) { Xr[12 + j] = Q::ld(P.Xbar, kx + 6 + j, 3); Xr[15 + j] = Q::ld(P.Xbar, kx + 24 + j, 3); Ur[j] = Q::ld(P.Ubar, ku + j, 3); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) _Pragma("unroll") for (int c = 0; c < 36; c++) Kr[j][c] = Q::ld(P.K, kg + j + 12 * c, 3);
    };
    int pi = 0, k = 0;
    _Pragma("nounroll")
    for (int s = 0; s < n_steps; s++) {
        pi = wbs_uniform(map[s]); k = wbs_uniform(map[n_steps + s]);
        const int reset = wbs_uniform(map[2 * n_steps + s]);
        PhaseC& P = ph[pi];
        const int h = P.h;
        const size_t kx = ((size_t)b * (h + 1) + k) * 36, ku = ((size_t)b * h + k) * 12, kg = ((size_t)b * h + k) * 432;
        // ---- disturbed walk: the push, then the noise of this step - drawn here and consumed by the feedback below, so that nothing of it lives
        // across the contact solve.  Every switch is a wave-uniform branch.  The twelve base entries of the estimate error are the same in the
        // four lanes: lane l draws three of them (positions 0..2, 3..5, velocities 0..2, 3..5) and the quad reads them by broadcasts (every lane
        // drawing all twelve: 24.8 ms against 19.9 ms, same measurement).
        WbsMcArgs mc; S nz_b[3], nz_q[3], nz_v[3], nz_u[3];
        if constexpr (D::MC) {
            mc = *wbs_mc_fresh(dist.a);
            if (s == mc.kick_step) {
                const typename Q::B on = Q::gt(alive, S(0.5));
                _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::sel(on, qb[i] + Q::ld(mc.kick, g * 36 + i, 0), qb[i]); vb[i] = Q::sel(on, vb[i] + Q::ld(mc.kick, g * 36 + 18 + i, 0), vb[i]); }
                _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::sel(on, ql[j] + Q::ld(mc.kick, g * 36 + 6 + j, 3), ql[j]); vl[j] = Q::sel(on, vl[j] + Q::ld(mc.kick, g * 36 + 24 + j, 3), vl[j]); }
            }
            if constexpr (D::NOISE) {
                const unsigned long long base = ((mc.first_problem + (unsigned long long)b) * 65536ull + (unsigned long long)(g - (size_t)b * (size_t)mc.R)) * 65536ull + (unsigned long long)s;
                if (mc.sq > 0.0 || mc.sv > 0.0) {
                    wbs_mc_normal3(mc.seed, base, Q::legc(12.0, 15.0, 30.0, 33.0), nz_b);
                    const S sg = Q::legc(mc.sq, mc.sq, mc.sv, mc.sv);
                    _Pragma("unroll") for (int j = 0; j < 3; j++) nz_b[j] = sg * nz_b[j];
                }
                if (mc.sq > 0.0) { wbs_mc_normal3(mc.seed, base, Q::legc(18.0, 21.0, 24.0, 27.0), nz_q); _Pragma("unroll") for (int j = 0; j < 3; j++) nz_q[j] = mc.sq * nz_q[j]; }
                if (mc.sv > 0.0) { wbs_mc_normal3(mc.seed, base, Q::legc(36.0, 39.0, 42.0, 45.0), nz_v); _Pragma("unroll") for (int j = 0; j < 3; j++) nz_v[j] = mc.sv * nz_v[j]; }
                if (mc.su > 0.0) { wbs_mc_normal3(mc.seed, base, Q::legc(0.0, 3.0, 6.0, 9.0), nz_u); _Pragma("unroll") for (int j = 0; j < 3; j++) nz_u[j] = mc.su * nz_u[j]; }
            }
        }
        // ---- feedback: the lane forms the three torques of its leg, rows 3 lane .. 3 lane + 2 of K (12 x 36, column-major) times x - xbar.  The
        // base part of x - xbar is in every lane already, the other legs' parts come by quad broadcasts.
        S ul[3];
        {
#if SIM_PREFETCH
            if (s == 0) fetch(P, kx, ku, kg);      // (later knots: fetched ahead of the previous knot's contact solve, below)
#else
            fetch(P, kx, ku, kg);
#endif
            S eb[6], wb[6], el[3], wl[3];
            _Pragma("unroll") for (int i = 0; i < 6; i++) { eb[i] = qb[i] - Xr[i]; wb[i] = vb[i] - Xr[6 + i]; }
            _Pragma("unroll") for (int j = 0; j < 3; j++) { el[j] = ql[j] - Xr[12 + j]; wl[j] = vl[j] - Xr[15 + j]; }
            record(eb, wb, el, wl);
            if constexpr (D::MC) {      // the fall test on the recorded state; then the policy sees the estimate x + e
                if (mc.fall > 0.0) ffall = Q::sel(Q::gt(alive * Q::sel(Q::gt(zero, ffall), one, zero) * Q::sel(Q::gt(S(mc.fall), qb[2]), one, zero), S(0.5)), S((double)s), ffall);
                if (D::NOISE && mc.sq > 0.0) {
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { eb[j] = eb[j] + Q::template get<0>(nz_b[j]); eb[3 + j] = eb[3 + j] + Q::template get<1>(nz_b[j]); el[j] = el[j] + nz_q[j]; }
                }
                if (D::NOISE && mc.sv > 0.0) {
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { wb[j] = wb[j] + Q::template get<2>(nz_b[j]); wb[3 + j] = wb[3 + j] + Q::template get<3>(nz_b[j]); wl[j] = wl[j] + nz_v[j]; }
                }
            }
            S dx[36];
            _Pragma("unroll") for (int i = 0; i < 6; i++) { dx[i] = eb[i]; dx[18 + i] = wb[i]; }
            _Pragma("unroll") for (int j = 0; j < 3; j++) {
                dx[6 + j] = Q::template get<0>(el[j]); dx[9 + j] = Q::template get<1>(el[j]); dx[12 + j] = Q::template get<2>(el[j]); dx[15 + j] = Q::template get<3>(el[j]);
                dx[24 + j] = Q::template get<0>(wl[j]); dx[27 + j] = Q::template get<1>(wl[j]); dx[30 + j] = Q::template get<2>(wl[j]); dx[33 + j] = Q::template get<3>(wl[j]);
            }
            S um = zero;
            _Pragma("unroll")
            for (int j = 0; j < 3; j++) {
                S acc = Kr[j][0] * dx[0];
                _Pragma("unroll") for (int c = 1; c < 36; c++) acc = acc + Kr[j][c] * dx[c];
                ul[j] = Ur[j] + acc;
                if constexpr (D::MC) {      // the actuator: noise on the commanded torque, then the limit
                    if (D::NOISE && mc.su > 0.0) ul[j] = ul[j] + nz_u[j];
                    if (mc.umax > 0.0) {
                        const S lim = S(mc.umax);
                        nsat = nsat + Q::sel(Q::gt(alive * Q::sel(Q::gt(wbs_abs<Q, S>(ul[j]), lim), one, zero), S(0.5)), one, zero);
                        ul[j] = Q::sel(Q::gt(ul[j], lim), lim, Q::sel(Q::gt(-lim, ul[j]), -lim, ul[j]));
                    }
                }
                um = wbs_max<Q, S>(um, wbs_abs<Q, S>(ul[j]));
            }
            umax = Q::sel(Q::gt(alive, S(0.5)), wbs_max<Q, S>(umax, um), umax);
        }
#if SIM_PREFETCH
        if (s + 1 < n_steps) {      // the next knot's rows do not depend on the state: their loads go out before the contact solve of this one
            const int pn = wbs_uniform(map[s + 1]), kn = wbs_uniform(map[n_steps + s + 1]);
            PhaseC& N = ph[pn];
            fetch(N, ((size_t)b * (N.h + 1) + kn) * 36, ((size_t)b * N.h + kn) * 12, ((size_t)b * N.h + kn) * 432);
        }
#endif
        if (trajX != nullptr) store_state((g * (size_t)(n_steps + 1) + s) * 36);
        if (trajU != nullptr) { _Pragma("unroll") for (int j = 0; j < 3; j++) Q::st(trajU, (g * (size_t)n_steps + s) * 12 + j, 3, ul[j]); }
        // ---- the step, and behind the last knot of a phase with a touchdown the impact: ONE call site of the dynamics, the phase boundary is a
        // uniform branch of the loop.  Sub-stepped walk: S trips of the step with the same torques, then the impact - S + reset trips, the last one
        // in mode 1 when reset is set.  A quad that diverged in an earlier trip rides along through the rest (the selects below keep its state).
        const int cm_dyn = (P.contact[0] > 0 ? 1 : 0) | (P.contact[1] > 0 ? 2 : 0) | (P.contact[2] > 0 ? 4 : 0) | (P.contact[3] > 0 ? 8 : 0);
        const int cm_td = (P.td[0] ? 1 : 0) | (P.td[1] ? 2 : 0) | (P.td[2] ? 4 : 0) | (P.td[3] ? 8 : 0);
        const double dt = P.dt, alpha = P.bg_alpha;
        if constexpr (D::UNI) {
            // ---- unilateral contact: the state machine of the head of the file.  stg: 0 the first solve of a substep (the landing test follows it), 1 the
            // landing impact, 2 a solve again, 3 the scheduled reset map.  stg and sub are wave-uniform: they change on ballots only.
            auto flag = [](int m) { return Q::legc((m & 1) ? 1.0 : 0.0, (m & 2) ? 1.0 : 0.0, (m & 4) ? 1.0 : 0.0, (m & 8) ? 1.0 : 0.0); };      // the lane's bit of a wave-uniform mask, formed at every use
            fr = Q::sel(Q::gt(alive, S(0.5)), fr * flag(cm_dyn), fr);      // F <- F n C: does something at a phase change only
            if constexpr (D::TER) er = Q::sel(Q::gt(alive, S(0.5)), er * (one - flag(cm_dyn)), er);      // E <- E \ C: such a foot is an ordinary attached stance foot now
            if constexpr (D::FRIC) fs(FRIC_SL) = Q::sel(Q::gt(alive, S(0.5)), fs(FRIC_SL) * (flag(cm_dyn) * (one - fr) + (one - flag(cm_dyn)) * er), fs(FRIC_SL));      // Sl <- Sl n A: a foot that left the stance set leaves Sl
            int sub = 0, stg = 0;
            _Pragma("nounroll")
            for (;;) {
                const int mode = (stg == 1 || stg == 3) ? 1 : 0;
                typename wbs_io_pick<D::FRIC != 0, D::PLANT != 0, D::TER != 0, S>::type io;
                io.cl = stg == 1 ? tl : stg == 3 ? flag(cm_td) : flag(cm_dyn) * (one - fr);
                if constexpr (D::TER) { if (mode == 0) io.cl = io.cl + (one - flag(cm_dyn)) * er; }      // A = (C \ F) u E
                if constexpr (D::FRIC) {      // the lane's friction column, read by the solve where it needs it, and the sample's row of the table
                    const WbsFricArgs fa = *wbs_fric_fresh(dist.fc);
                    io.col = fcell.col; io.stride = fcell.stride; io.mur = fa.mu + 2 * (size_t)fa.mu_of[g]; io.vstick = fa.v_stick;
                }
                S ob[6]; V3<S> ol;
                if constexpr (D::PLANT) {      // the quad's row: inertias for the solve, gain and friction on the torque it is given
                    const WbsPlantArgs pa = *wbs_plant_fresh(dist.pl);
                    io.row = pa.P + (size_t)pa.plant_of[g] * SIM_PLANT_ROW;
                    S ue[3];
                    _Pragma("unroll") for (int j = 0; j < 3; j++) ue[j] = Q::ld(io.row, 22 + j, 3) * ul[j] - Q::ld(io.row, 34 + j, 3) * vl[j];
                    park(true, ul);
                    wbs_contact_dynamics<Q>(md, 0, mode, mode == 0 ? 1e-12 : 0.0, alpha, qb, vb, ql, vl, ue, ob, ol, &io);
                } else {
                park(true, ul);
                wbs_contact_dynamics<Q>(md, 0, mode, mode == 0 ? 1e-12 : 0.0, alpha, qb, vb, ql, vl, ul, ob, ol, &io);
                }
                park(false, ul);
                if (mode != 0) {      // positions stay, velocities jump: the scheduled reset map for every live sample, a landing for the quads that have one
                    const typename Q::B on = Q::gt(alive * (stg == 3 ? one : Q::sum(tl)), S(0.5));
                    const S o3[3] = {ol.x, ol.y, ol.z};
                    _Pragma("unroll") for (int i = 0; i < 6; i++) vb[i] = Q::sel(on, ob[i], vb[i]);
                    _Pragma("unroll") for (int j = 0; j < 3; j++) vl[j] = Q::sel(on, o3[j], vl[j]);
                    if (stg == 3) break;
                    if constexpr (D::TER) {      // T n C leaves F as before; T \ C joins E
                        const S ts = tl * flag(cm_dyn), te = tl - ts;
                        fr = fr - ts; nland = nland + ts; er = er + te; nearly = nearly + te;
                        efirst = Q::sel(Q::gt(Q::sum(te) * Q::sel(Q::gt(zero, efirst), one, zero), S(0.5)), S((double)s), efirst);
                    } else {
                    fr = fr - tl; nland = nland + tl;      // (T holds feet of live samples only)
                    }
                    stg = 2;
                    continue;
                }
                const WbsUniArgs ua = *wbs_uni_fresh(dist.un);
                S att = flag(cm_dyn) * (one - fr);      // the set this solve ran on
                if constexpr (D::TER) att = att + (one - flag(cm_dyn)) * er;
                if (stg == 0) {      // landing test at the substep's start state, over the free scheduled stance feet of a live sample
                    const S fc = alive * fr;
                    const typename Q::B isf = Q::gt(fc, S(0.5));
                    if constexpr (!D::TER) {
                    mlift = Q::sel(isf, wbs_max<Q, S>(mlift, io.pz - ua.z_ground), mlift);
                    tl = fc * Q::sel(Q::gt(io.pz, S(ua.z_ground)), zero, one) * Q::sel(Q::gt(zero, io.wz), one, zero);
                    } else {      // the same test against the looked-up height, and over the swing feet outside E with the threshold -w_td
                        const WbsTerArgs ta = *wbs_ter_fresh(dist.te);
                        const S zg = ua.z_ground + wbs_ter_height(ta, ta.map_of[g], io.px, io.py);
                        const S sw = alive * (ta.early != 0 ? one : zero) * (one - flag(cm_dyn)) * (one - er);
                        const S below = Q::sel(Q::gt(io.pz, zg), zero, one);
                        mlift = Q::sel(isf, wbs_max<Q, S>(mlift, io.pz - zg), mlift);
                        tl = fc * below * Q::sel(Q::gt(zero, io.wz), one, zero) + sw * below * Q::sel(Q::gt(S(-ta.w_td), io.wz), one, zero);
                        mpen = Q::sel(Q::gt(tl, S(0.5)), wbs_max<Q, S>(mpen, zg - io.pz), mpen);
                    }
                    if (wbs_any(Q::sum(tl))) { stg = 1; continue; }
                }
                if constexpr (D::FRIC) {      // a sliding foot the solve found at rest was held with three rows: it leaves Sl (a repeat of the solve sees a sticking foot).
                                              // Behind the landing test: a solve whose wave goes on to a landing impact decides nothing
                    const S rs = alive * att * fs(FRIC_SL) * (one - fs(FRIC_EFF));
                    fs(FRIC_SL) = fs(FRIC_SL) - rs; fs(FRIC_NRESTICK) = fs(FRIC_NRESTICK) + rs;
                }
                {   // lift-off test: the attached foot with the smallest normal force, lowest leg on a tie, if that force is below fz_rel
                    const S lz = Q::sel(Q::gt(att, S(0.5)), io.lam.z, S(HUGE_VAL)), mz = Q::vmin(lz);
                    const S need = alive * Q::sel(Q::gt(S(ua.fz_rel), mz), one, zero);
                    if (wbs_any(need)) {
                        const S lane = Q::legc(0.0, 1.0, 2.0, 3.0);
                        const S pick = Q::vmin(Q::sel(Q::gt(lz, mz), S(4.0), lane));
                        const S rel = need * Q::sel(Q::gt(wbs_abs<Q, S>(lane - pick), S(0.5)), zero, one);
                        if constexpr (D::TER) {      // a stance foot goes into F, a foot of E simply leaves E
                            const S rs = rel * flag(cm_dyn), re = rel - rs;
                            fr = fr + rs; nrel = nrel + rs; er = er - re; nerel = nerel + re;
                            ufirst = Q::sel(Q::gt(Q::sum(rs) * Q::sel(Q::gt(zero, ufirst), one, zero), S(0.5)), S((double)s), ufirst);
                            if constexpr (D::FRIC) { fs(FRIC_SL) = fs(FRIC_SL) * (one - rel); fs(FRIC_FRESH) = fs(FRIC_FRESH) * (one - rel); }      // a released foot leaves Sl
                        } else {
                        fr = fr + rel; nrel = nrel + rel;
                        ufirst = Q::sel(Q::gt(need * Q::sel(Q::gt(zero, ufirst), one, zero), S(0.5)), S((double)s), ufirst);
                        }
                        stg = 2;
                        continue;
                    }
                }
                if constexpr (D::FRIC) {      // onset test, reached only when no quad of the wave released a foot: the sticking attached foot with the smallest cone margin
                    const WbsFricArgs fa = *wbs_fric_fresh(dist.fc);
                    const S mus = S(fa.mu[2 * (size_t)fa.mu_of[g]]);
                    const S stick = att * (one - fs(FRIC_SL));
                    const S lt = wbs_sqrt(io.lam.x * io.lam.x + io.lam.y * io.lam.y);
                    const S mf = Q::sel(Q::gt(stick, S(0.5)), mus * io.lam.z - lt, S(HUGE_VAL)), mm = Q::vmin(mf);
                    const S ons = alive * Q::sel(Q::gt(zero, mm), one, zero);
                    if (wbs_any(ons)) {
                        const S lane = Q::legc(0.0, 1.0, 2.0, 3.0);
                        const S pick = Q::vmin(Q::sel(Q::gt(mf, mm), S(4.0), lane));
                        const typename Q::B join = Q::gt(ons * Q::sel(Q::gt(wbs_abs<Q, S>(lane - pick), S(0.5)), zero, one), S(0.5));
                        const typename Q::B pull = Q::gt(lt, zero);      // (lambda_t = 0: the foot leaves the cone through its tip and has no direction)
                        const S rl = Q::rcp(lt);
                        fs(FRIC_SL) = Q::sel(join, one, fs(FRIC_SL)); fs(FRIC_FRESH) = Q::sel(join, one, fs(FRIC_FRESH)); fs(FRIC_NF) = Q::sel(join, wbs_max<Q, S>(io.lam.z, zero), fs(FRIC_NF));
                        fs(FRIC_TX) = Q::sel(join, Q::sel(pull, io.lam.x * rl, zero), fs(FRIC_TX)); fs(FRIC_TY) = Q::sel(join, Q::sel(pull, io.lam.y * rl, zero), fs(FRIC_TY));
                        fs(FRIC_NONSET) = fs(FRIC_NONSET) + Q::sel(join, one, zero);
                        fs(FRIC_FIRST) = Q::sel(Q::gt(ons * Q::sel(Q::gt(zero, fs(FRIC_FIRST)), one, zero), S(0.5)), S((double)s), fs(FRIC_FIRST));
                        stg = 2;
                        continue;
                    }
                }
                {   // ---- the last solve of the substep.  Records as below, over the ATTACHED feet; a free foot's force is exactly zero
                    const WbsGrfArgs ga = *wbs_grf_fresh(dist.gr);
                    const typename Q::B isa = Q::gt(att, S(0.5));
                    V3<S> lam_ = {Q::sel(isa, io.lam.x, zero), Q::sel(isa, io.lam.y, zero), Q::sel(isa, io.lam.z, zero)};
                    S cfl = alive * att;      // the feet whose cone margin counts: with friction the STICKING attached feet
                    if constexpr (D::FRIC) {      // a sliding foot's force is (f_t, lambda_z); end of the substep: n_f, the fresh flags and the row's running values
                        const S sl = fs(FRIC_SL);
                        const typename Q::B isl = Q::gt(alive * att * sl, S(0.5));
                        lam_.x = Q::sel(Q::gt(att * sl, S(0.5)), fs(FRIC_FX), lam_.x); lam_.y = Q::sel(Q::gt(att * sl, S(0.5)), fs(FRIC_FY), lam_.y);
                        cfl = alive * att * (one - sl);
                        const S wx = fs(FRIC_WX), wy = fs(FRIC_WY), wt = wbs_sqrt(wx * wx + wy * wy);
                        const double hs_ = dt / (double)wbs_uniform(wbs_sub_fresh(dist.sb)->substeps);
                        fs(FRIC_NF) = Q::sel(isl, wbs_max<Q, S>(io.lam.z, zero), fs(FRIC_NF));
                        fs(FRIC_FRESH) = Q::sel(Q::gt(alive, S(0.5)), zero, fs(FRIC_FRESH));
                        fs(FRIC_NSLIDE) = fs(FRIC_NSLIDE) + Q::sel(isl, one, zero); fs(FRIC_DIST) = fs(FRIC_DIST) + Q::sel(isl, wt * hs_, zero); fs(FRIC_VMAX) = Q::sel(isl, wbs_max<Q, S>(fs(FRIC_VMAX), wt), fs(FRIC_VMAX));
                    }
                    const V3<S> lam = lam_;
                    const typename Q::B on = Q::gt(alive * att, S(0.5));
                    const S cone = ga.mu * lam.z - wbs_max<Q, S>(wbs_abs<Q, S>(lam.x), wbs_abs<Q, S>(lam.y));
                    const S bad = wbs_max<Q, S>(Q::sel(Q::gt(S(ga.fz_min), lam.z), one, zero), Q::sel(Q::gt(zero, cone), one, zero));
                    const typename Q::B slip = Q::gt(cfl * bad, S(0.5));
                    gfmin = Q::sel(on, Q::min(gfmin, lam.z), gfmin); gcmin = Q::sel(Q::gt(cfl, S(0.5)), Q::min(gcmin, cone), gcmin); gfmax = Q::sel(on, wbs_max<Q, S>(gfmax, lam.z), gfmax);
                    gfirst = Q::sel(slip, Q::min(gfirst, S((double)s)), gfirst); gslip = gslip + Q::sel(slip, one, zero);
                    nfree = nfree + alive * fr;
                    if constexpr (D::TER) nheld = nheld + alive * er;
                    if (ga.Y != nullptr && sub == 0) { Q::st(ga.Y, (g * (size_t)n_steps + s) * 12, 3, lam.x); Q::st(ga.Y, (g * (size_t)n_steps + s) * 12 + 1, 3, lam.y); Q::st(ga.Y, (g * (size_t)n_steps + s) * 12 + 2, 3, lam.z); }
                }
                const int nsub = wbs_uniform(wbs_sub_fresh(dist.sb)->substeps);
                {   // forward Euler with dt / S, then the divergence test on the new state (as below)
                    const double hs = dt / (double)nsub;
                    S xb[6], yb[6], xl[3], yl[3], nsq = zero;
                    _Pragma("unroll") for (int i = 0; i < 6; i++) { xb[i] = qb[i] + vb[i] * hs; yb[i] = vb[i] + ob[i] * hs; nsq = nsq + w0 * (xb[i] * xb[i] + yb[i] * yb[i]); }
                    const S o3[3] = {ol.x, ol.y, ol.z};
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { xl[j] = ql[j] + vl[j] * hs; yl[j] = vl[j] + o3[j] * hs; nsq = nsq + (xl[j] * xl[j] + yl[j] * yl[j]); }
                    nsq = Q::sum(nsq);
                    const S good = Q::sel(Q::gt(nsq, S(1e12)), zero, one) * Q::sel(Q::gt(nsq + 1.0, nsq), one, zero);
                    first_bad = Q::sel(Q::gt(alive * (one - good), S(0.5)), S((double)s), first_bad);
                    alive = alive * good;
                    const typename Q::B on = Q::gt(alive, S(0.5));
                    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::sel(on, xb[i], qb[i]); vb[i] = Q::sel(on, yb[i], vb[i]); }
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::sel(on, xl[j], ql[j]); vl[j] = Q::sel(on, yl[j], vl[j]); }
                }
                sub++; stg = 0;
                if (sub >= nsub) { if (reset != 0) stg = 3; else break; }
            }
        } else {
            int last = reset;
            if constexpr (D::SUB) last = reset + wbs_uniform(wbs_sub_fresh(dist.sb)->substeps) - 1;
            _Pragma("nounroll")
            for (int trip = 0; trip <= last; trip++) {
                int mode = trip;
                if constexpr (D::SUB) mode = (reset != 0 && trip == last) ? 1 : 0;
                S ob[6]; V3<S> ol;
                park(true, ul);
                if constexpr (D::GRF) {
                    V3<S> lam;
                    if constexpr (D::PLANT) {      // as in the walk with the contact rule; the contact flag is the lane's bit of the wave-uniform mask
                        const WbsPlantArgs pa = *wbs_plant_fresh(dist.pl);
                        const int cm = mode == 0 ? cm_dyn : cm_td;
                        WbsPlantIO<S> io;
                        io.cl = Q::legc((cm & 1) ? 1.0 : 0.0, (cm & 2) ? 1.0 : 0.0, (cm & 4) ? 1.0 : 0.0, (cm & 8) ? 1.0 : 0.0);
                        io.row = pa.P + (size_t)pa.plant_of[g] * SIM_PLANT_ROW;
                        S ue[3];
                        _Pragma("unroll") for (int j = 0; j < 3; j++) ue[j] = Q::ld(io.row, 22 + j, 3) * ul[j] - Q::ld(io.row, 34 + j, 3) * vl[j];
                        wbs_contact_dynamics<Q>(md, 0, mode, mode == 0 ? 1e-12 : 0.0, alpha, qb, vb, ql, vl, ue, ob, ol, &io);
                        lam = io.lam;
                    } else {
                    wbs_contact_dynamics<Q>(md, mode == 0 ? cm_dyn : cm_td, mode, mode == 0 ? 1e-12 : 0.0, alpha, qb, vb, ql, vl, ul, ob, ol, &lam);
                    }
                    park(false, ul);
                    // ---- records: the force of the step on the lane's foot, counted if the foot is a stance foot of the phase (a select on the
                    // wave-uniform contact mask) and the sample had not diverged before the step (`alive` is still the value the step began with).
                    // The impact takes no record.
                    if (mode == 0) {
                        const WbsGrfArgs ga = *wbs_grf_fresh(dist.gr);
                        const S st = Q::legc((cm_dyn & 1) ? 1.0 : 0.0, (cm_dyn & 2) ? 1.0 : 0.0, (cm_dyn & 4) ? 1.0 : 0.0, (cm_dyn & 8) ? 1.0 : 0.0);
                        const typename Q::B on = Q::gt(alive * st, S(0.5));
                        const S cone = ga.mu * lam.z - wbs_max<Q, S>(wbs_abs<Q, S>(lam.x), wbs_abs<Q, S>(lam.y));
                        const S bad = wbs_max<Q, S>(Q::sel(Q::gt(S(ga.fz_min), lam.z), one, zero), Q::sel(Q::gt(zero, cone), one, zero));
                        const typename Q::B slip = Q::gt(alive * st * bad, S(0.5));
                        gfmin = Q::sel(on, Q::min(gfmin, lam.z), gfmin); gcmin = Q::sel(on, Q::min(gcmin, cone), gcmin); gfmax = Q::sel(on, wbs_max<Q, S>(gfmax, lam.z), gfmax);
                        gfirst = Q::sel(slip, Q::min(gfirst, S((double)s)), gfirst); gslip = gslip + Q::sel(slip, one, zero);
                        if (ga.Y != nullptr && (D::SUB == 0 || trip == 0)) { Q::st(ga.Y, (g * (size_t)n_steps + s) * 12, 3, lam.x); Q::st(ga.Y, (g * (size_t)n_steps + s) * 12 + 1, 3, lam.y); Q::st(ga.Y, (g * (size_t)n_steps + s) * 12 + 2, 3, lam.z); }
                    }
                } else {
                    wbs_contact_dynamics<Q>(md, mode == 0 ? cm_dyn : cm_td, mode, mode == 0 ? 1e-12 : 0.0, alpha, qb, vb, ql, vl, ul, ob, ol);
                    park(false, ul);
                }
                if (mode == 0) {      // forward Euler (WBM.cpp:25-26), then the divergence test on the new state
                    double hs = dt;       // (substeps) the step of a trip, dt / S: one division, formed where it is used
                    if constexpr (D::SUB) hs = dt / (double)wbs_uniform(wbs_sub_fresh(dist.sb)->substeps);
                    S xb[6], yb[6], xl[3], yl[3], nsq = zero;
                    _Pragma("unroll") for (int i = 0; i < 6; i++) { xb[i] = qb[i] + vb[i] * hs; yb[i] = vb[i] + ob[i] * hs; nsq = nsq + w0 * (xb[i] * xb[i] + yb[i] * yb[i]); }
                    const S o3[3] = {ol.x, ol.y, ol.z};
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { xl[j] = ql[j] + vl[j] * hs; yl[j] = vl[j] + o3[j] * hs; nsq = nsq + (xl[j] * xl[j] + yl[j] * yl[j]); }
                    nsq = Q::sum(nsq);
                    // good <=> !(nsq > 1e12) && nsq == nsq   (below 1e12 adding one always gives a larger number; a NaN compares false)
                    const S good = Q::sel(Q::gt(nsq, S(1e12)), zero, one) * Q::sel(Q::gt(nsq + 1.0, nsq), one, zero);
                    first_bad = Q::sel(Q::gt(alive * (one - good), S(0.5)), S((double)s), first_bad);
                    alive = alive * good;
                    const typename Q::B on = Q::gt(alive, S(0.5));
                    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::sel(on, xb[i], qb[i]); vb[i] = Q::sel(on, yb[i], vb[i]); }
                    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::sel(on, xl[j], ql[j]); vl[j] = Q::sel(on, yl[j], vl[j]); }
                } else {              // reset map: positions stay, velocities jump
                    const typename Q::B on = Q::gt(alive, S(0.5));
                    const S o3[3] = {ol.x, ol.y, ol.z};
                    _Pragma("unroll") for (int i = 0; i < 6; i++) vb[i] = Q::sel(on, ob[i], vb[i]);
                    _Pragma("unroll") for (int j = 0; j < 3; j++) vl[j] = Q::sel(on, o3[j], vl[j]);
                }
            }
        }
    }
    {   // the state behind the last step, against the knot that follows it
        PhaseC& P = ph[pi];
        S eb[6], wb[6], el[3], wl[3];
        deviation(P, ((size_t)b * (P.h + 1) + k + 1) * 36, eb, wb, el, wl);
        record(eb, wb, el, wl);
    }
    if constexpr (D::MC) {      // the final state takes the fall test with index n_steps
        const WbsMcArgs mc = *wbs_mc_fresh(dist.a);
        if (mc.fall > 0.0) ffall = Q::sel(Q::gt(alive * Q::sel(Q::gt(zero, ffall), one, zero) * Q::sel(Q::gt(S(mc.fall), qb[2]), one, zero), S(0.5)), S((double)n_steps), ffall);
        Q::st0(mc.extra, g * 2, ffall); Q::st0(mc.extra, g * 2 + 1, Q::sum(nsat));
    }
    if constexpr (D::GRF) {      // the quad's record: the four feet joined (first_slip: the earliest; none: -1)
        const WbsGrfArgs ga = *wbs_grf_fresh(dist.gr);
        const S first = Q::vmin(gfirst);
        Q::st0(ga.rows, g * SIM_GRF_ROW, Q::vmin(gfmin)); Q::st0(ga.rows, g * SIM_GRF_ROW + 1, Q::vmin(gcmin)); Q::st0(ga.rows, g * SIM_GRF_ROW + 2, wbs_qmax<Q, S>(gfmax));
        Q::st0(ga.rows, g * SIM_GRF_ROW + 3, Q::sel(Q::gt(first, S(0.5 * SIM_GRF_NONE)), S(-1.0), first)); Q::st0(ga.rows, g * SIM_GRF_ROW + 4, Q::sum(gslip));
    }
    if constexpr (D::UNI) {      // the quad's contact row: the four feet joined; free_final: bit l = leg l is free; then F back to where it came from
        const WbsUniArgs ua = *wbs_uni_fresh(dist.un);
        const S top = wbs_qmax<Q, S>(mlift);
        Q::st0(ua.rows, g * SIM_UNI_ROW, ufirst); Q::st0(ua.rows, g * SIM_UNI_ROW + 1, Q::sum(nrel)); Q::st0(ua.rows, g * SIM_UNI_ROW + 2, Q::sum(nland));
        Q::st0(ua.rows, g * SIM_UNI_ROW + 3, Q::sum(nfree)); Q::st0(ua.rows, g * SIM_UNI_ROW + 4, Q::sum(fr * Q::legc(1.0, 2.0, 4.0, 8.0)));
        Q::st0(ua.rows, g * SIM_UNI_ROW + 5, Q::sel(Q::gt(S(-1e300), top), zero, top));
        if (ua.F != nullptr && (ua.hold == nullptr || ua.hold[g * (size_t)ua.hold_stride] == 0)) Q::st(ua.F, g * 4, 1, fr);
        if constexpr (D::TER) {      // the terrain row, and E back to where it came from under the same hold
            const WbsTerArgs ta = *wbs_ter_fresh(dist.te);
            const S deep = wbs_qmax<Q, S>(mpen);
            Q::st0(ta.rows, g * SIM_TER_ROW, efirst); Q::st0(ta.rows, g * SIM_TER_ROW + 1, Q::sum(nearly)); Q::st0(ta.rows, g * SIM_TER_ROW + 2, Q::sum(nerel));
            Q::st0(ta.rows, g * SIM_TER_ROW + 3, Q::sum(nheld)); Q::st0(ta.rows, g * SIM_TER_ROW + 4, Q::sum(er * Q::legc(1.0, 2.0, 4.0, 8.0)));
            Q::st0(ta.rows, g * SIM_TER_ROW + 5, Q::sel(Q::gt(S(-1e300), deep), zero, deep));
            if (ta.E != nullptr && (ua.hold == nullptr || ua.hold[g * (size_t)ua.hold_stride] == 0)) Q::st(ta.E, g * 4, 1, er);
        }
        if constexpr (D::FRIC) {      // the friction row; Sl and n_f back to where they came from under the same hold
            const WbsFricArgs fa = *wbs_fric_fresh(dist.fc);
            Q::st0(fa.rows, g * SIM_FRIC_ROW, fs(FRIC_FIRST)); Q::st0(fa.rows, g * SIM_FRIC_ROW + 1, Q::sum(fs(FRIC_NONSET))); Q::st0(fa.rows, g * SIM_FRIC_ROW + 2, Q::sum(fs(FRIC_NSLIDE)));
            Q::st0(fa.rows, g * SIM_FRIC_ROW + 3, Q::sum(fs(FRIC_NRESTICK))); Q::st0(fa.rows, g * SIM_FRIC_ROW + 4, Q::sum(fs(FRIC_SL) * Q::legc(1.0, 2.0, 4.0, 8.0)));
            Q::st0(fa.rows, g * SIM_FRIC_ROW + 5, wbs_qmax<Q, S>(fs(FRIC_VMAX))); Q::st0(fa.rows, g * SIM_FRIC_ROW + 6, Q::sum(fs(FRIC_DIST)));
            if (fa.Sl != nullptr && (ua.hold == nullptr || ua.hold[g * (size_t)ua.hold_stride] == 0)) { Q::st(fa.Sl, g * 4, 1, fs(FRIC_SL)); Q::st(fa.NF, g * 4, 1, fs(FRIC_NF)); }
        }
    }
    if (trajX != nullptr) store_state((g * (size_t)(n_steps + 1) + n_steps) * 36);
    _Pragma("unroll") for (int i = 0; i < 6; i++) { Q::st0(xfinal, g * 36 + i, qb[i]); Q::st0(xfinal, g * 36 + 18 + i, vb[i]); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { Q::st(xfinal, g * 36 + 6 + j, 3, ql[j]); Q::st(xfinal, g * 36 + 24 + j, 3, vl[j]); }
    Q::st0(rows, g * SIM_ROW, wbs_qmax<Q, S>(dq)); Q::st0(rows, g * SIM_ROW + 1, wbs_qmax<Q, S>(dv)); Q::st0(rows, g * SIM_ROW + 2, hmin);
    Q::st0(rows, g * SIM_ROW + 3, wbs_qmax<Q, S>(umax)); Q::st0(rows, g * SIM_ROW + 4, first_bad);
}

// The pending reset map of an episode (epi_impact of episode.hpp) on the robot's own plant: the same program with the inertias of row plant_of[g].  An
// impact takes no torque, so gain and friction do not enter.  frozen[g stride] != 0: the robot's episode has ended - its quad computes with the others
// and stores nothing.
template <class Q> HD void wbs_plant_impact(PhaseC* ph, const ModelDev& md, int pi, size_t g, const int* frozen, int stride, double* state, double* x0, const WbsPlantArgs* pl) {
    using S = typename Q::S;
    PhaseC& P = ph[pi];
    S qb[6], vb[6], ql[3], vl[3], ul[3], ob[6]; V3<S> ol;
    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::ld(state, g * 36 + i, 0); vb[i] = Q::ld(state, g * 36 + 18 + i, 0); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::ld(state, g * 36 + 6 + j, 3); vl[j] = Q::ld(state, g * 36 + 24 + j, 3); ul[j] = S(0.0); }
    WbsPlantIO<S> io;
    io.cl = Q::legc(P.td[0] ? 1.0 : 0.0, P.td[1] ? 1.0 : 0.0, P.td[2] ? 1.0 : 0.0, P.td[3] ? 1.0 : 0.0);
    io.row = pl->P + (size_t)pl->plant_of[g] * SIM_PLANT_ROW;
    wbs_contact_dynamics<Q>(md, 0, 1, 0.0, P.bg_alpha, qb, vb, ql, vl, ul, ob, ol, &io);
    if (frozen[g * (size_t)stride] != 0) return;
    const S o3[3] = {ol.x, ol.y, ol.z};
    _Pragma("unroll") for (int i = 0; i < 6; i++) { Q::st0(state, g * 36 + 18 + i, ob[i]); Q::st0(x0, g * 36 + i, qb[i]); Q::st0(x0, g * 36 + 18 + i, ob[i]); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { Q::st(state, g * 36 + 24 + j, 3, o3[j]); Q::st(x0, g * 36 + 6 + j, 3, ql[j]); Q::st(x0, g * 36 + 24 + j, 3, o3[j]); }
}

#if !defined(HS_HOST_EMU)
// The kernels.  grid = ceil(B R / 16) waves of sixteen quads.  The loop is sequential in the knots, so a launch has B R / 16 waves whatever the window length.
#ifndef SIM_WPE
#define SIM_WPE 1      // waves per SIMD the kernel is compiled for (as k_rollout_quad: up to 512 registers)
#endif
// Every walk is this wrapper around wbs_walk: 64 lanes, one wave per SIMD, lane t parks in column t of `stash` (PARK doubles per lane: the sum of the
// SIM_*_PARK of what the policy carries), and a quad leaves or stays as a whole.  PARAMS: the kernel's parameters behind the eleven common ones, WBS_P(...)
// or nothing; the variadic tail: the same names, as the members of POLICY.  Names, types and order of the parameters are part of the mangled kernel
// names, which the profiles and `make resources` key on.
#define WBS_P(...) , __VA_ARGS__
#define WBS_KERNEL(NAME, POLICY, PARK, PARAMS, ...)                                                                                                                            \
    __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))                                                                               \
    NAME(const PhaseDev* ph_, ModelDev md, const int* map, int n_steps, int n_samples, int total, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU \
         PARAMS) {                                                                                                                                                             \
        __shared__ double stash[(PARK) * 64];                                                                                                                                  \
        const int g = blockIdx.x * 16 + (threadIdx.x >> 2);                                                                                                                    \
        if (g >= total) return;                                                                                                                                                \
        wbs_walk<QS, POLICY>((PhaseC*)ph_, md, map, n_steps, g / n_samples, (size_t)g, x0, xfinal, rows, trajX, trajU, stash, POLICY{__VA_ARGS__});                            \
    }

// One launch of a walk, host side: the stream, the grid, the eleven common kernel arguments, which kernel (sim_pick.hpp) and the blocks of switches in
// device memory that its policy points at (those of switches the pick leaves out are not read).
struct WbsLaunch {
    hipStream_t stream; unsigned grid;
    const PhaseDev* ph; const ModelDev* md; const int* map; int n_steps, n_samples, total; const double* x0; double *xfinal, *rows, *trajX, *trajU;
    SimPick pick;
    const WbsMcArgs* mc; const WbsGrfArgs* gr; const WbsSubArgs* sb; const WbsUniArgs* un; const WbsTerArgs* te; const WbsPlantArgs* pl;
    const WbsFricArgs* fc = nullptr;      // (hsddp_friction.h) read by the friction family alone
};
template <class K, class... A> void wbs_launch(const WbsLaunch& L, K kernel, A... policy_args) {
    hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(64), 0, L.stream, L.ph, *L.md, L.map, L.n_steps, L.n_samples, L.total, L.x0, L.xfinal, L.rows, L.trajX, L.trajU, policy_args...);
}
// The launcher of each family (SimFamily): it picks among its kernels by L.pick and launches one.  None of them looks at the runtime's error state: a
// launch that fails is reported by the caller's hipGetLastError (reading the error here would reset it and hide the failure from that check).
void wbs_base_launch(const WbsLaunch& L);       // below
void wbs_sub_launch(const WbsLaunch& L);        // hsddp_sub.hip
void wbs_uni_launch(const WbsLaunch& L);        // hsddp_uni.hip
void wbs_ter_launch(const WbsLaunch& L);        // hsddp_ter.hip
void wbs_plant_launch(const WbsLaunch& L);      // hsddp_plant.hip
void wbs_fric_launch(const WbsLaunch& L);       // hsddp_fric.hip
void wbs_plant_impact_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const ModelDev& md, int pi, int total, const int* frozen, int stride, double* state, double* x0,
                             const WbsPlantArgs* pl);

#if !defined(HS_SIM_WALK_ONLY)      // (HS_SIM_WALK_ONLY: hsddp_sub.hip and the like take the walk and the macro and instantiate kernels of their own)
// The plain walk; the disturbed walk (hsddp_mc_run: mc points at the run's switches in device memory; k_sim_quad_mc draws noise, k_sim_quad_mc0 is the
// walk of a run without any, see WbsMc); and the twins of the three with contact-force records (hsddp_grf_set: gr points at the thresholds and the
// destinations in device memory).
WBS_KERNEL(k_sim_quad, WbsPlain, SIM_PARK, , )
WBS_KERNEL(k_sim_quad_mc, WbsMc<1>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc)
WBS_KERNEL(k_sim_quad_mc0, WbsMc<0>, SIM_PARK_MC, WBS_P(const WbsMcArgs* mc), mc)
WBS_KERNEL(k_sim_quad_grf, WbsGrf, SIM_PARK + SIM_GRF_PARK, WBS_P(const WbsGrfArgs* gr), gr)
WBS_KERNEL(k_sim_quad_mc_grf, WbsMcGrf<1>, SIM_PARK_MC + SIM_GRF_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr), mc, gr)
WBS_KERNEL(k_sim_quad_mc0_grf, WbsMcGrf<0>, SIM_PARK_MC + SIM_GRF_PARK, WBS_P(const WbsMcArgs* mc, const WbsGrfArgs* gr), mc, gr)
// The sub-stepped walks (hsddp_substep_set with S > 1) are six more instantiations with SUB 1 in the policy: hsddp_sub.hip, a translation unit of its own.
// The walks with unilateral ground contact (hsddp_contact_set) are three more with UNI 1: hsddp_uni.hip, likewise; so are hsddp_ter.hip and hsddp_plant.hip.
void wbs_base_launch(const WbsLaunch& L) {
    const bool noise = L.pick.variant == SIM_VAR_MC;
    if (!L.pick.records) {
        if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad);
        else wbs_launch(L, noise ? k_sim_quad_mc : k_sim_quad_mc0, L.mc);
    } else {
        if (L.pick.variant == SIM_VAR_PLAIN) wbs_launch(L, k_sim_quad_grf, L.gr);
        else wbs_launch(L, noise ? k_sim_quad_mc_grf : k_sim_quad_mc0_grf, L.mc, L.gr);
    }
}
#endif
#endif

}  // namespace hs
