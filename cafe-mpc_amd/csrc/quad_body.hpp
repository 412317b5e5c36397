// The body of k_rollout_quad (hsddp_quad.hip) and k_rollout_quad_pw (hsddp_pw.hip): the whole-body running knots on lane quads (the kernel's
// description is in hsddp_quad.hip).  This file is the TEXT between the kernel's braces: it is included there, once per kernel, and reads the
// kernel's parameters by their names (ph_, slot_phase, slot_k, qslots, nq, nslots, batch, md, el, opt, x0, sa, st, mask, fail, units, plist, nlist).
// Text and not a function template like quad_term_body because k_rollout_quad has to keep compiling to the instructions it compiles to (its register
// allocation fills the file at one wave per SIMD), and the same statements behind a call boundary come out of the optimiser in another order.
// QUAD_BODY_PW (set by the includer, 0 or 1): per-problem cost-weight scales (hsddp_weights.h) - the kernel has one more parameter, wtab = the handle's
// table [batch][84], and a lane reads the row of its own quad's problem.  QUAD_BODY_LIM (0 or 1, with QUAD_BODY_PW): per-problem constraint limits
// (hsddp_limits.h) - one more parameter again, ltab = the handle's resolved table [phase][batch][12]; a lane reads row (phase, its problem).  No include guard on purpose; it needs wb_quad.hpp, rollout_args.hpp and
// quad_term_body.hpp (QS_* row offsets) in front of the kernel.
    PhaseC* ph = (PhaseC*)ph_;
    __shared__ double stage[16 * QS_ROW];
    // plist / nlist: the problems this launch is for (null: all of the batch, `mask` picks).  A probe launch of a line search or a commit launch only
    // concerns some problems; packed sixteen to a wave from the list the deciding kernel left behind, its waves are full whatever the share is
    const int nprob = plist != nullptr ? nlist : batch;
    const int nbg = (nprob + 15) >> 4;
    const int qi = blockIdx.x / nbg, bg = blockIdx.x - qi * nbg;
    const int s = qslots[qi], pi = slot_phase[s], k = slot_k[s];
    PhaseC& P = ph[pi];
    const int t = threadIdx.x;
    const int ix = bg * 16 + (t >> 2);
    const int b = ix < nprob ? (plist != nullptr ? plist[ix] : ix) : batch;
    const bool active = b < batch && !masked_out(st[b < batch ? b : 0], mask);
    {   // knots this launch rolls out (measurement only): one atomic per wave, every candidate of the loop counted
        const unsigned long long m = __ballot(active && (t & 3) == 0);
        if (m == 0) return;      // none of the wave's problems takes part in this launch (a masked launch over the whole batch): nothing to stage
        if (t == 0) atomicAdd(units, (unsigned long long)(__popcll(m) * el.n));
    }
    {   // stage the rows of the wave's sixteen problems: per problem three whole-wave loads (Xbar, dX, reference row: entries 0..63) and one that
        // gathers the six tails; all of them issued before the first is written to LDS.  A group that is only partly filled (nprob no multiple of 16)
        // stages its last problem again in the empty places, so nothing is read beyond the list or the batch.
        const int h = P.h;
        const HS_GLOBAL double *pX = P.Xbar, *pdX = P.dX, *pU = P.Ubar, *pdU = P.dU, *pKdX = P.KdX, *pR = P.rref;
        const int seg = t < 8 ? 0 : t < 16 ? 1 : t < 28 ? 2 : t < 40 ? 3 : t < 52 ? 4 : 5;      // tail of Xbar, dX (entries 64..71), Ubar, dU, K dX, reference row (64..75)
        const int toff = seg == 0 ? 64 + t : seg == 1 ? 64 + (t - 8) : seg == 2 ? t - 16 : seg == 3 ? t - 28 : seg == 4 ? t - 40 : 64 + (t - 52);      // entry within its array's row
        const int tdst = seg == 0 ? toff : seg == 1 ? QS_DX + toff : seg == 2 ? QS_U + toff : seg == 3 ? QS_DU + toff : seg == 4 ? QS_KDX + toff : QS_RR + toff;
        // the tails' source as ONE address form for every lane, base + (problem x rows-per-problem + knot's row + entry): the lane's array is picked here, once
        const HS_GLOBAL double* tsrc = seg == 0 ? pX : seg == 1 ? pdX : seg == 2 ? pU : seg == 3 ? pdU : seg == 4 ? pKdX : pR;
        const unsigned tmul = seg < 2 ? (unsigned)(h + 1) * 36u : seg < 5 ? (unsigned)h * 12u : (unsigned)P.ref_pb * 80u;
        const size_t tadd = (size_t)k * (seg < 2 ? 36 : seg < 5 ? 12 : 80) + toff;
        const int ixl = min(bg * 16 + (t & 15), nprob - 1);
        const int bl = plist != nullptr ? plist[ixl] : ixl;      // lane p (mod 16) holds problem p of the group
        double v[16][4];
        _Pragma("unroll")
        for (int p = 0; p < 16; p++) {
            const int bp = __builtin_amdgcn_readlane(bl, p);
            const size_t kx = ((size_t)bp * (h + 1) + k) * 36, kr = ref_row(P, bp, k) * 80;
            v[p][0] = pX[kx + t]; v[p][1] = pdX[kx + t]; v[p][2] = pR[kr + t]; v[p][3] = tsrc[(size_t)bp * tmul + tadd];
        }
        _Pragma("unroll")
        for (int p = 0; p < 16; p++) {
            double* row = stage + p * QS_ROW;
            row[t] = v[p][0]; row[QS_DX + t] = v[p][1]; row[QS_RR + t] = v[p][2]; row[tdst] = v[p][3];
        }
    }
    QDL::lane_slot()[t] = t & 3;
    __syncthreads();      // (one wave: orders the LDS writes above before the other lanes' reads below)
    if (!active) return;      // (a quad leaves or stays as a whole: the cross-lane steps below need all four lanes)
    _Pragma("nounroll")
    for (int c = 0; c < el.n; c++) {      // el.writer is the last candidate of a launch or none: `wr` is uniform over the wave in every trip
        // Every trip starts from a descriptor pointer, a problem, a knot and a row offset the compiler cannot see through: nothing a trip reads
        // or derives from them (its LDS rows, the descriptor's scalars, addresses) may be hoisted out of the loop and held in registers across
        // it - the knot's live set has no room for that (QDL, wb_quad.hpp, does the same for what depends on the lane).
        PhaseC* Pc = &P; HS_PIN_S(Pc);
        int bc = b, kc = k; HS_PIN_S(kc);
        int ro = (t >> 2) * QS_ROW; HS_PIN(bc); HS_PIN(ro);
        const HS_LDS double* row = (const HS_LDS double*)stage + ro;
        const QuadIn<const HS_LDS double*> in = {row, row + QS_DX, row + QS_U, row + QS_DU, row + QS_KDX, row + QS_RR};
        const double eps = el.from_state ? st[bc].ls_eps : el.e[c];
#if defined(QUAD_BODY_LIM) && QUAD_BODY_LIM
        const QuadOut q = wbq_rollout_knot<QDL, true, true>(*Pc, md, bc, kc, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, c == el.writer, in, (WsRow)wtab + (size_t)bc * WS_ROW,
                                                            (LimRow)ltab + ((size_t)pi * batch + bc) * LIM_ROW);
#elif QUAD_BODY_PW
        const QuadOut q = wbq_rollout_knot<QDL, true>(*Pc, md, bc, kc, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, c == el.writer, in, (WsRow)wtab + (size_t)bc * WS_ROW);
#else
        const QuadOut q = wbq_rollout_knot<QDL>(*Pc, md, bc, kc, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, c == el.writer, in);
#endif
        if ((t & 3) == 0) {
            const size_t slot = ((size_t)c * batch + bc) * nslots + s;
            sa.cost[slot] = q.cost; sa.dsq[slot] = q.dsq; sa.ming[slot] = q.ming; sa.maxh[slot] = 0.0;
            if (q.bad) fail[(size_t)c * batch + bc] = 1;
        }
    }
