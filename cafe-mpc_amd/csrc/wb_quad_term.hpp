// Whole-body TERMINAL knot on a LANE QUAD: wb_rollout_terminal (wb_knot.hpp) restated for the mapping of wb_quad.hpp - one lane per leg, sixteen
// problems per wave.
//
// The terminal knot of a phase is its state at k = h, the terminal cost and touchdown constraint there, and the reset map into the next phase
// (MHPCReset.cpp:4-28): the impact on the feet that touch down, then the successor's Xsim[0] and Defect[0].  On the one-wave program it keeps 12-23 of
// 64 lanes busy like the running knot did; here it is
//   * the state and the reference row from the caller's rows (QuadIn: xbar / dx hold knot h in [0, 36) and knot 0 of the SUCCESSOR in [36, 72));
//   * ONE pass down the leg with the velocities only (no accelerations, no link forces: the terminal knot has no bias term) for the foot's position
//     and velocity;
//   * the terminal cost: tracking, foot-placement regularisation, touchdown-velocity penalty, added in the reference's order between the quantities
//     (wb_terminal_cost_base); the AL terms of the touchdown feet one by one in foot order (the one-wave program's lane 0 does the same);
//   * only when the phase ends in an impact: composite inertias, mass-matrix blocks, foot Jacobian, block factor and the block impulse solve on the
//     touchdown feet - the contact solve of wbq_rollout_knot in mode 1 (impulseDynamics, WBM.cpp:178-206, 427-456):
//         lam = G^-1 (-Jc v),  v+ = v + L^-T X lam,  no damping, no right-hand side from the bias forces (y = 0)
//     which is what wbs_contact_dynamics (wb_sim.hpp) computes with mode = 1.  COPIED from there, like that one from wbq_rollout_knot and for the same
//     reason: the simulation kernels and k_rollout_quad have to keep compiling to what they compile to.  A change to the dynamics has to be made in
//     all three (tests/test_quad_terminal_host.py holds this copy against the one-wave program).
// The caller owns a terminal slot only when the successor - if there is one - is a whole-body phase with a shooting node at knot 0 (split_slots,
// hsddp_hip.hip): no projection to another model, no single-shooting chain to walk.  The terminal knot raises no flag (neither does the one-wave one).
#pragma once
#include "wb_quad.hpp"

namespace hs {

struct QuadTermOut { double cost, dsq, maxh; };

// Terminal knot of problem b of phase P (whole-body, with shooting nodes), step length eps, evaluated by a lane quad.  Pn: the successor (whole-body
// with shooting nodes) or null behind the last phase.
//   wr = false: a probe - only (Phi, defect^2 of the successor's knot 0, max |h|) come back;  wr = true additionally stores what wb_rollout_terminal
//   stores: X[h], Phibase, Phi, th and the successor's Xsim[0], Defect[0].  wr must be uniform over the wave.
//   in: xbar / dx rows of 72 (knot h, then knot 0 of the successor - unread without one), rr: row h of the packed references.
//   TDH: the lane's foot is held to the problem's own height tdh[leg] (hsddp_touchdown.h: tdh points at the problem's four) instead of ground_height.
//   PW: the tracking weights are qf[j] sqf[j] of the scale row ws of the lane's problem (hsddp_weights.h), read with the state.
template <class Q, bool TDH = false, bool PW = false, class PT>
HD QuadTermOut wbq_rollout_terminal(PhaseC& P, PhaseC* Pn, const ModelDev& md, int b, double eps, int al_active, bool wr, const QuadIn<PT>& in, const double* tdh = nullptr,
                                    WsRow ws = nullptr) {
    using S = typename Q::S;
    const bool WR = wr;
    const int h = P.h;
    const size_t kx = ((size_t)b * (h + 1) + h) * 36;
    const S zero = S(0.0);
    const S w0 = Q::legc(1.0, 0.0, 0.0, 0.0);      // the replicated base entries are counted once
    // ---- state of the knot: the floating base replicated in every lane, the lane's own leg
    S qb[6], vb[6], ql[3], vl_[3];
    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::ld(in.xbar, i, 0) + eps * Q::ld(in.dx, i, 0); vb[i] = Q::ld(in.xbar, 18 + i, 0) + eps * Q::ld(in.dx, 18 + i, 0); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::ld(in.xbar, 6 + j, 3) + eps * Q::ld(in.dx, 6 + j, 3); vl_[j] = Q::ld(in.xbar, 24 + j, 3) + eps * Q::ld(in.dx, 24 + j, 3); }
    if (WR) {
        _Pragma("unroll") for (int j = 0; j < 3; j++) {
            Q::st(P.X, kx + 6 + j, 3, ql[j]); Q::st(P.X, kx + 24 + j, 3, vl_[j]);
            Q::st0(P.X, kx + j, qb[j]); Q::st0(P.X, kx + 3 + j, qb[3 + j]); Q::st0(P.X, kx + 18 + j, vb[j]); Q::st0(P.X, kx + 21 + j, vb[3 + j]);
        }
    }
    const PT rr = in.rr;
    S sqb[6], svb[6], sql[3], svl[3];      // PW: scales of the base entries (positions, velocities) and of the lane's leg
    if constexpr (PW) {
        _Pragma("unroll") for (int i = 0; i < 6; i++) { sqb[i] = Q::ld(ws, WS_QF + i, 0); svb[i] = Q::ld(ws, WS_QF + 18 + i, 0); }
        _Pragma("unroll") for (int j = 0; j < 3; j++) { sql[j] = Q::ld(ws, WS_QF + 6 + j, 3); svl[j] = Q::ld(ws, WS_QF + 24 + j, 3); }
    }
    // ---- terminal tracking cost (QuadraticTrackingCost, MHPCCost.cpp:67-87): needs the state only
    S Phi;
    {
        S sxq = zero;
        _Pragma("unroll")
        for (int i = 0; i < 6; i++) {
            const S dq = qb[i] - Q::ld(rr, i, 0), dv = vb[i] - Q::ld(rr, 18 + i, 0);
            if constexpr (PW) { const S wq = P.qf[i] * sqb[i], wv = P.qf[18 + i] * svb[i]; sxq = sxq + w0 * (dq * wq * dq + dv * wv * dv); }
            else sxq = sxq + w0 * (dq * P.qf[i] * dq + dv * P.qf[18 + i] * dv);
        }
        _Pragma("unroll")
        for (int j = 0; j < 3; j++) {
            const S dq = ql[j] - Q::ld(rr, 6 + j, 3), dv = vl_[j] - Q::ld(rr, 24 + j, 3);
            S wq = Q::legc(P.qf[6 + j], P.qf[9 + j], P.qf[12 + j], P.qf[15 + j]), wv = Q::legc(P.qf[24 + j], P.qf[27 + j], P.qf[30 + j], P.qf[33 + j]);
            if constexpr (PW) { wq = wq * sql[j]; wv = wv * svl[j]; }
            sxq = sxq + (dq * wq * dq + dv * wv * dv);
        }
        Phi = 0.5 * Q::sum(sxq);
    }
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
    // ---- foot position and velocity: the velocity half of the bias pass of wbq_rollout_knot, down the leg
    V3<S> fpos, fvel;
    V3<S> rB;      // foot relative to the trunk origin, trunk axes (for the Jacobian below)
    V3<S> dA, dH;  // foot relative to the abad origin (trunk axes after Rx) / hip origin, A axes
    {
        V3<S> om = {zero, zero, zero}, vl = {vb[0], vb[1], vb[2]};
        auto revj = [&](auto AXT, const S& c, const S& s, const S& qd, V3<S>& om_, V3<S>& vl_2) {
            constexpr int AX = decltype(AXT)::value;
            V3<S> o = rotT<AX>(c, s, om_), v = rotT<AX>(c, s, vl_2);
            if (AX == 0) o.x = o.x + qd;
            if (AX == 1) o.y = o.y + qd;
            if (AX == 2) o.z = o.z + qd;
            om_ = o; vl_2 = v;
        };
        using A0 = IC<0>; using A1 = IC<1>; using A2 = IC<2>;
        revj(A2{}, T.c3, T.s3, vb[3], om, vl); revj(A1{}, T.c4, T.s4, vb[4], om, vl); revj(A0{}, T.c5, T.s5, vb[5], om, vl);
        V3<S> o1 = om, v1 = vl + cross(om, pa);
        revj(A0{}, ca, sa, vl_[0], o1, v1);
        V3<S> o2 = o1, v2 = v1 + cross(o1, ph);
        o2 = rotT<2>(S(cps), S(sps), o2); v2 = rotT<2>(S(cps), S(sps), v2);
        revj(A1{}, ch, sh, vl_[1], o2, v2);
        V3<S> o3 = o2, v3 = v2 + cross(o2, pk);
        revj(A1{}, ck, sk, vl_[2], o3, v3);
        // foot point (0, 0, -0.195) in K: velocity, position
        const V3<S> rf = {zero, zero, S(-0.195)};
        V3<S> w = v3 + cross(o3, rf);      // K -> world
        w = rot<1>(ck, sk, w); w = rot<1>(ch, sh, w); w = rot<2>(S(cps), S(sps), w); w = rot<0>(ca, sa, w);
        w = rot<0>(T.c5, T.s5, w); w = rot<1>(T.c4, T.s4, w); w = rot<2>(T.c3, T.s3, w);
        fvel = w;
        const V3<S> rK = rot<1>(ck, sk, rf);                            // foot relative to the knee origin, H axes
        const V3<S> rH = pk + rK;                                       // ... relative to the hip origin, H axes
        dH = rot<2>(S(cps), S(sps), rot<1>(ch, sh, rH));                // ... relative to the hip origin, A axes
        const V3<S> rA = ph + dH;                                       // ... relative to the abad origin, A axes
        dA = rot<0>(ca, sa, rA);                                        // ... relative to the abad origin, trunk axes
        rB = pa + dA;
        const V3<S> rW = rot<2>(T.c3, T.s3, rot<1>(T.c4, T.s4, rot<0>(T.c5, T.s5, rB)));
        fpos = V3<S>{qb[0], qb[1], qb[2]} + rW;
    }
    // ---- touchdown feet: flag of the lane's leg, its rank among them (= its terminal-constraint index)
    const S cl = Q::legc(P.td[0] ? 1.0 : 0.0, P.td[1] ? 1.0 : 0.0, P.td[2] ? 1.0 : 0.0, P.td[3] ? 1.0 : 0.0);
    const typename Q::B on = Q::gt(cl, S(0.5));
    const S cf0 = Q::template get<0>(cl), cf1 = Q::template get<1>(cl), cf2 = Q::template get<2>(cl);
    const S before = Q::legc(0, 1, 0, 0) * cf0 + Q::legc(0, 0, 1, 0) * (cf0 + cf1) + Q::legc(0, 0, 0, 1) * (cf0 + cf1 + cf2);
    // ---- foot terms of the terminal cost (MHPCCost.cpp:255-268): foot-placement regulariser of the reference's stance feet, touchdown-velocity penalty
    {
        const S rel[3] = {Q::ld(rr, 64, 3), Q::ld(rr, 65, 3), Q::ld(rr, 66, 3)};
        const S rc = Q::ld(rr, 60, 1);
        const V3<S> d = {(fpos.x - qb[0]) - rel[0], (fpos.y - qb[1]) - rel[1], (fpos.z - qb[2]) - rel[2]};
        const S wr0 = P.w_foot_reg[0], wr1 = P.w_foot_reg[1], wr2 = P.w_foot_reg[2], wtd = P.w_td_vel;
        const S t2 = 0.5 * (d.x * wr0 * d.x + d.y * wr1 * d.y + d.z * wr2 * d.z), t5 = 0.5 * fvel.z * wtd * fvel.z;
        const S l2 = Q::sum(Q::sel(Q::gt(rc, S(0.0)), (P.w_foot_reg[0] >= 0) ? t2 : zero, zero));
        const S l5 = Q::sum(Q::sel(on, (P.n_td > 0 && P.w_td_vel >= 0) ? t5 : zero, zero));
        Phi = Phi + l2; Phi = Phi + l5;
    }
    if (WR) Q::st0(P.Phibase, (size_t)b, Phi);
    // ---- touchdown constraint (height of the touchdown feet above the ground) and its AL terms, foot by foot in foot order
    S maxh = zero;
    if (P.nt > 0) {
        const size_t tb = (size_t)b * P.nt;
        const S ti = Q::sel(on, before, S(0.0));      // (a lane without a touchdown reads a valid dummy and contributes nothing)
        const S sg = Q::ldv(P.sigma, tb, ti), lm = Q::ldv(P.lambda, tb, ti);
        S hh;
        if constexpr (TDH) hh = fpos.z - Q::ld(tdh, 0, 1); else hh = fpos.z - P.ground_height;
        if (WR) Q::stv(P.th, tb, ti, on, hh);
        maxh = -Q::vmin(Q::sel(on, Q::sel(Q::gt(zero, hh), hh, -hh), zero));      // max |h| over the touchdown feet
        S c = zero;
        auto al_foot = [&](auto JT) {
            constexpr int J = decltype(JT)::value;
            if (P.td[J]) { const S hf = Q::template get<J>(hh), sf = Q::template get<J>(sg), lf = Q::template get<J>(lm); c = c + 0.5 * sf * hf * hf; c = c + lf * hf; }
        };
        al_foot(IC<0>{}); al_foot(IC<1>{}); al_foot(IC<2>{}); al_foot(IC<3>{});
        if (al_active) Phi = Phi + c;
    }
    if (WR) Q::st0(P.Phi, (size_t)b, Phi);
    QuadTermOut out;
    out.cost = Q::lane0(Phi); out.maxh = Q::lane0(maxh); out.dsq = 0.0;
    if (Pn == nullptr) return out;
    // ---- reset map (MHPCReset.cpp:4-28): impact if any foot touches down, v+ = v without one
    S vpb[6]; V3<S> vpl;
    if (P.has_impact) {
        // composite inertias, leg -> trunk (frames: K shank, H thigh, A abad, B trunk; v_H = Ry(qk) v_K, v_A = Rz(psi) Ry(qh) v_H, v_B = Rx(qa) v_A)
        const RBI<S> IK = rbi_link<S>(0.064, zero, zero, S(-0.061), S(0.000245), zero, zero, S(0.000248), zero, S(0.000006));
        RBI<S> IH = rbi_link<S>(0.634, zero, sy * 0.016, S(-0.02), S(0.001983), sy * 0.000245, S(0.000013), S(0.002103), sy * 0.0000015, S(0.000408));
        IH = rbi_add(IH, rbi_shift(IK.m, rot<1>(ck, sk, IK.h), sym_rot<1>(ck, sk, IK.I), pk));
        RBI<S> IA = rbi_link<S>(0.54, zero, sy * 0.036, zero, S(0.000381), sy * 0.000058, S(0.00000045), S(0.000560), sy * 0.00000095, S(0.000444));
        IA = rbi_add(IA, rbi_shift(IH.m, rot<2>(S(cps), S(sps), rot<1>(ch, sh, IH.h)), sym_rot<2>(S(cps), S(sps), sym_rot<1>(ch, sh, IH.I)), ph));
        const RBI<S> IBl = rbi_shift(IA.m, rot<0>(ca, sa, IA.h), sym_rot<0>(ca, sa, IA.I), pa);
        // whole robot about the trunk origin: trunk + the four legs (sums over the quad)
        RBI<S> IT;
        IT.m = Q::sum(IBl.m) + 3.3; IT.h = {Q::sum(IBl.h.x), Q::sum(IBl.h.y), Q::sum(IBl.h.z)};
        IT.I = {Q::sum(IBl.I.xx) + 0.011253, Q::sum(IBl.I.xy), Q::sum(IBl.I.xz), Q::sum(IBl.I.yy) + 0.036203, Q::sum(IBl.I.yz), Q::sum(IBl.I.zz) + 0.042673};
        // mass-matrix blocks of the leg: D (3x3, joints abad / hip / knee) and Ct[c][j] = M(base joint c, leg joint j)
        S Ct[6][3], d_aa, d_ha, d_hh, d_ka, d_kh, d_kk;
        {
            V3<S> n = {IK.I.xy, IK.I.yy, IK.I.yz}, f = {IK.h.z, zero, -IK.h.x};                               // knee: unit acceleration about y of K
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
        // base block B (6x6, replicated): unit accelerations of the base joints seen in trunk axes, force of the WHOLE robot, walked back
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
        // foot Jacobian of the leg, world axes: Ja (3 x 3 over abad, hip, knee), Jb (3 x 6 over the base joints) - geometric form axis x arm
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
        // factor of M, block form.  L = [ blockdiag(L_l) 0 ; E  L_S ],  E_l = Ct L_l^-T (6 x 3),  S = B - sum_l E_l E_l^T
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
        // X = L^-1 Jc^T for the lane's foot (zero for a foot that does not touch down): Xt (3 leg rows x 3 force directions), Xb (6 base rows x 3)
        M33<S> Xt; S Xb[6][3];      // Xt.r[d] = column d (force direction d) as a 3-vector over the leg rows ; Xb[c][d]
        _Pragma("unroll")
        for (int d = 0; d < 3; d++) {
            const V3<S> xt = scale(cl, fwd3(Ll, Ja.r[d]));      // L_l^-1 (row d of Ja)^T
            Xt.r[d] = xt;
            S w[6];
            _Pragma("unroll") for (int c = 0; c < 6; c++) w[c] = cl * Jb[d][c] - (E[c][0] * xt.x + E[c][1] * xt.y + E[c][2] * xt.z);
            fwd6(LS, rdS, w);
            _Pragma("unroll") for (int c = 0; c < 6; c++) Xb[c][d] = w[c];
        }
        // Gram matrix G = X^T X in 3 x 3 blocks: lane f holds block row f (blocks g <= f); the diagonal block of a foot outside the set is the identity
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
        {   // the lane's own diagonal block: + Xt^T Xt (touchdown) / identity (not in the set)
            M33<S> Gd;
            const S dg = 1.0 - cl;
            _Pragma("unroll")
            for (int r = 0; r < 3; r++) {
                const S e0 = dot3(Xt.r[r], Xt.r[0]), e1 = dot3(Xt.r[r], Xt.r[1]), e2 = dot3(Xt.r[r], Xt.r[2]);
                Gd.r[r] = {e0 + (r == 0 ? dg : zero), e1 + (r == 1 ? dg : zero), e2 + (r == 2 ? dg : zero)};
            }
            const S m0 = Q::legc(1, 0, 0, 0), m1 = Q::legc(0, 1, 0, 0), m2 = Q::legc(0, 0, 1, 0), m3 = Q::legc(0, 0, 0, 1);
            _Pragma("unroll")
            for (int r = 0; r < 3; r++) {
                G[0].r[r] = G[0].r[r] + scale(m0, Gd.r[r]); G[1].r[r] = G[1].r[r] + scale(m1, Gd.r[r]);
                G[2].r[r] = G[2].r[r] + scale(m2, Gd.r[r]); G[3].r[r] = G[3].r[r] + scale(m3, Gd.r[r]);
            }
        }
        // right-hand side -Jc v: J v of a foot is its velocity
        V3<S> rhs = {cl * (-fvel.x), cl * (-fvel.y), cl * (-fvel.z)};
        // block Cholesky of G over the quad (no damping: impulseDynamics): block column kc is finished by lane kc, then lanes f > kc form L_f,kc
        M33<S> Lg[4]; Chol3<S> Ld;      // Lg[g]: block (own lane, g) of the factor, g < own lane ; Ld: the own diagonal block's factor
        {
            const S lane = Q::legc(0, 1, 2, 3);
            auto bcast33 = [&](auto JT, const M33<S>& A) { constexpr int J = decltype(JT)::value; M33<S> o; _Pragma("unroll") for (int r = 0; r < 3; r++) o.r[r] = {Q::template get<J>(A.r[r].x), Q::template get<J>(A.r[r].y), Q::template get<J>(A.r[r].z)}; return o; };
            auto bcastL = [&](auto JT, const Chol3<S>& A) { constexpr int J = decltype(JT)::value; Chol3<S> o; o.l10 = Q::template get<J>(A.l10); o.l20 = Q::template get<J>(A.l20); o.l21 = Q::template get<J>(A.l21); o.r0 = Q::template get<J>(A.r0); o.r1 = Q::template get<J>(A.r1); o.r2 = Q::template get<J>(A.r2); return o; };
            auto sub_abt = [&](M33<S>& A, const M33<S>& Pm, const M33<S>& Qm) { _Pragma("unroll") for (int r = 0; r < 3; r++) A.r[r] = A.r[r] - V3<S>{dot3(Pm.r[r], Qm.r[0]), dot3(Pm.r[r], Qm.r[1]), dot3(Pm.r[r], Qm.r[2])}; };
            auto right_solve = [&](M33<S>& A, const Chol3<S>& Lk) { _Pragma("unroll") for (int r = 0; r < 3; r++) { V3<S> a = A.r[r], x; x.x = a.x * Lk.r0; x.y = (a.y - x.x * Lk.l10) * Lk.r1; x.z = (a.z - x.x * Lk.l20 - x.y * Lk.l21) * Lk.r2; A.r[r] = x; } };
            auto own_diag = [&](const M33<S>& Gk) { return chol3<Q, S>(Gk.r[0].x, Gk.r[1].x, Gk.r[1].y, Gk.r[2].x, Gk.r[2].y, Gk.r[2].z); };
            Chol3<S> L0 = own_diag(G[0]);                       // meaningful in lane 0
            const Chol3<S> L00 = bcastL(J0{}, L0);
            Lg[0] = G[0]; right_solve(Lg[0], L00);              // lanes 1..3: L_f0
            const M33<S> L10 = bcast33(J1{}, Lg[0]);
            M33<S> A1 = G[1]; sub_abt(A1, Lg[0], L10);          // lanes >= 1: G_f1 - L_f0 L_10^T
            Chol3<S> L1 = own_diag(A1);                         // meaningful in lane 1
            const Chol3<S> L11 = bcastL(J1{}, L1);
            Lg[1] = A1; right_solve(Lg[1], L11);                // lanes 2..3: L_f1
            const M33<S> L20 = bcast33(J2{}, Lg[0]), L21 = bcast33(J2{}, Lg[1]);
            M33<S> A2 = G[2]; sub_abt(A2, Lg[0], L20); sub_abt(A2, Lg[1], L21);
            Chol3<S> L2 = own_diag(A2);                         // meaningful in lane 2
            const Chol3<S> L22 = bcastL(J2{}, L2);
            Lg[2] = A2; right_solve(Lg[2], L22);                // lane 3: L_32
            M33<S> A3 = G[3]; sub_abt(A3, Lg[0], Lg[0]); sub_abt(A3, Lg[1], Lg[1]); sub_abt(A3, Lg[2], Lg[2]);      // lane 3: G_33 - sum L_3g L_3g^T
            Chol3<S> L3 = own_diag(A3);                         // meaningful in lane 3
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
            V3<S> lam3 = bwd3(Ld, z);                                             // valid in lane 3
            const V3<S> w32 = bc3(J3{}, m33_mulT(Lg[2], lam3)), w31 = bc3(J3{}, m33_mulT(Lg[1], lam3)), w30 = bc3(J3{}, m33_mulT(Lg[0], lam3));
            V3<S> lam2 = bwd3(Ld, z - w32);                                       // valid in lane 2
            const V3<S> w21 = bc3(J2{}, m33_mulT(Lg[1], lam2)), w20 = bc3(J2{}, m33_mulT(Lg[0], lam2));
            V3<S> lam1 = bwd3(Ld, z - w31 - w21);                                 // valid in lane 1
            const V3<S> w10 = bc3(J1{}, m33_mulT(Lg[0], lam1));
            V3<S> lam0 = bwd3(Ld, z - w30 - w20 - w10);                           // valid in lane 0
            rhs = {pick(lam0.x, lam1.x, lam2.x, lam3.x), pick(lam0.y, lam1.y, lam2.y, lam3.y), pick(lam0.z, lam1.z, lam2.z, lam3.z)};
        }
        const V3<S> lam = scale(cl, rhs);      // impulse on the lane's foot (world axes); zero for a foot that does not touch down
        // v+ = v + L^-T X lam: base part replicated, leg part in the lane
        _Pragma("unroll") for (int c = 0; c < 6; c++) vpb[c] = Q::sum(Xb[c][0] * lam.x + Xb[c][1] * lam.y + Xb[c][2] * lam.z);
        bwd6(LS, rdS, vpb);
        const V3<S> zl = {Xt.r[0].x * lam.x + Xt.r[1].x * lam.y + Xt.r[2].x * lam.z, Xt.r[0].y * lam.x + Xt.r[1].y * lam.y + Xt.r[2].y * lam.z, Xt.r[0].z * lam.x + Xt.r[1].z * lam.y + Xt.r[2].z * lam.z};
        S et[3];
        _Pragma("unroll") for (int j = 0; j < 3; j++) { S s = E[0][j] * vpb[0]; _Pragma("unroll") for (int c = 1; c < 6; c++) s = s + E[c][j] * vpb[c]; et[j] = s; }
        const V3<S> dvl = bwd3(Ll, zl - V3<S>{et[0], et[1], et[2]});
        _Pragma("unroll") for (int c = 0; c < 6; c++) vpb[c] = vpb[c] + vb[c];
        vpl = {dvl.x + vl_[0], dvl.y + vl_[1], dvl.z + vl_[2]};
    } else {
        _Pragma("unroll") for (int c = 0; c < 6; c++) vpb[c] = vb[c];
        vpl = {vl_[0], vl_[1], vl_[2]};
    }
    // ---- knot 0 of the successor: Xsim[0] = (q, v+), Defect[0] = Xsim[0] - (Xbar_n[0] + eps dX_n[0])
    PhaseC& N = *Pn;
    const size_t nx = (size_t)b * (N.h + 1) * 36;
    S dsq = zero;
    _Pragma("unroll")
    for (int i = 0; i < 6; i++) {
        const S d0 = qb[i] - (Q::ld(in.xbar, 36 + i, 0) + eps * Q::ld(in.dx, 36 + i, 0)), d1 = vpb[i] - (Q::ld(in.xbar, 54 + i, 0) + eps * Q::ld(in.dx, 54 + i, 0));
        dsq = dsq + w0 * (d0 * d0 + d1 * d1);
        if (WR) { Q::st0(N.Xsim, nx + i, qb[i]); Q::st0(N.Xsim, nx + 18 + i, vpb[i]); Q::st0(N.Defect, nx + i, d0); Q::st0(N.Defect, nx + 18 + i, d1); }
    }
    const S vp3[3] = {vpl.x, vpl.y, vpl.z};
    _Pragma("unroll")
    for (int j = 0; j < 3; j++) {
        const S d0 = ql[j] - (Q::ld(in.xbar, 42 + j, 3) + eps * Q::ld(in.dx, 42 + j, 3)), d1 = vp3[j] - (Q::ld(in.xbar, 60 + j, 3) + eps * Q::ld(in.dx, 60 + j, 3));
        dsq = dsq + (d0 * d0 + d1 * d1);
        if (WR) { Q::st(N.Xsim, nx + 6 + j, 3, ql[j]); Q::st(N.Xsim, nx + 24 + j, 3, vp3[j]); Q::st(N.Defect, nx + 6 + j, 3, d0); Q::st(N.Defect, nx + 24 + j, 3, d1); }
    }
    out.dsq = Q::lane0(Q::sum(dsq));
    return out;
}

#ifdef HS_HOST_EMU
// host form that gathers the rows from the phases' arrays (tests/_emu, one evaluation per knot)
template <class Q, bool TDH = false, bool PW = false>
inline QuadTermOut wbq_rollout_terminal(PhaseC& P, PhaseC* Pn, const ModelDev& md, int b, double eps, int al_active, bool wr, const double* tdh = nullptr, WsRow ws = nullptr) {
    double xb[72] = {0}, dx[72] = {0};
    const size_t kx = ((size_t)b * (P.h + 1) + P.h) * 36;
    for (int i = 0; i < 36; i++) { xb[i] = P.Xbar[kx + i]; dx[i] = P.dX[kx + i]; }
    if (Pn != nullptr) { const size_t nx = (size_t)b * (Pn->h + 1) * 36; for (int i = 0; i < 36; i++) { xb[36 + i] = Pn->Xbar[nx + i]; dx[36 + i] = Pn->dX[nx + i]; } }
    const QuadIn<const double*> in = {xb, dx, nullptr, nullptr, nullptr, P.rref + ref_row(P, b, P.h) * 80};
    return wbq_rollout_terminal<Q, TDH, PW>(P, Pn, md, b, eps, al_active, wr, in, tdh, ws);
}
#endif

}  // namespace hs
