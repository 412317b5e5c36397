// TEST-ONLY host build of the lane-quad TERMINAL knot (cafe-mpc_amd/csrc/wb_quad_term.hpp, the QH form: the four lanes of a quad as a four-wide
// value) beside the one-wave terminal knot (wb_knot.hpp) under the lane emulator.  It takes the whole emulator (emu.cpp: the handle, the ABI of
// include/hsddp.h, the per-step entry points that prepare a state worth evaluating) and adds the two terminal programs as entry points of their own,
// each with one step length PER PROBLEM (what a commit launch with `from_state` does), writing or probing.  tests/term_common.py builds and binds it.
#include "emu.cpp"
#include "wb_quad_term.hpp"

// the terminal slots the lane-quad path owns (split_slots, hsddp_hip.hip)
static bool term_owned(const hsddp_handle* h, int pi) {
    const PhaseDev& P = h->ph[pi];
    if (P.model != HSDDP_MODEL_WB || !P.shooting) return false;
    return pi + 1 >= h->nph || (h->ph[pi + 1].model == HSDDP_MODEL_WB && h->ph[pi + 1].shooting);
}

extern "C" {
// program 0: wb_rollout_terminal<64> (one wave); 1: wbq_rollout_terminal<QH>.  eps: [batch]; out: [batch][nph][4] = cost, defect^2, max |h|, min g of
// the terminal slot (NaN for a slot the quad path does not own).  wr = 0: a probe.
int term_emu_terminal(hsddp_handle_t* h, int program, const double* eps, const hsddp_option_t* opt, int wr, double* out) {
    static WbCore L;
    for (int b = 0; b < h->batch; b++) for (int pi = 0; pi < h->nph; pi++) {
        double* o = out + 4 * ((size_t)b * h->nph + pi);
        if (!term_owned(h, pi)) { o[0] = o[1] = o[2] = o[3] = NAN; continue; }
        const PhaseDev& P = h->ph[pi]; const PhaseDev* Pn = pi + 1 < h->nph ? &h->ph[pi + 1] : nullptr;
        if (program == 0) {
            double s4[4] = {NAN, NAN, NAN, NAN};
            SlotOut so{s4, s4 + 1, s4 + 3, s4 + 2};
            wb_rollout_terminal<64>(L, P, Pn, h->md, b, eps[b], opt->AL_active, so, 0, false, wr != 0);
            for (int q = 0; q < 4; q++) o[q] = s4[q];
        } else {
            const QuadTermOut q = wbq_rollout_terminal<QH>(P, Pn, h->md, b, eps[b], opt->AL_active, wr != 0);
            o[0] = q.cost; o[1] = q.dsq; o[2] = q.maxh; o[3] = 0.0;
        }
    }
    return 0;
}
// per-problem terminal records of a phase: out [batch][6] = Phibase, Phi, th[0..3] (NaN behind the phase's nt touchdown feet)
int term_emu_records(hsddp_handle_t* h, int pi, double* out) {
    const PhaseDev& P = h->ph[pi];
    for (int b = 0; b < h->batch; b++) {
        double* o = out + 6 * (size_t)b;
        o[0] = P.Phibase[b]; o[1] = P.Phi[b];
        for (int i = 0; i < 4; i++) o[2 + i] = i < P.nt ? P.th[(size_t)b * P.nt + i] : NAN;
    }
    return 0;
}
// AL parameters of the phase's touchdown constraint, per problem and touchdown foot: sigma = s0 + ds (b nt + i), lambda = l0 + dl (b nt + i)
int term_emu_set_al(hsddp_handle_t* h, int pi, double s0, double ds, double l0, double dl) {
    const PhaseDev& P = h->ph[pi];
    for (size_t i = 0; i < (size_t)h->batch * P.nt; i++) { P.sigma[i] = s0 + ds * (double)i; P.lambda[i] = l0 + dl * (double)i; }
    return P.nt;
}
}
