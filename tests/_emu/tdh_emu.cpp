// TEST-ONLY host build of the two terminal programs WITH per-problem touchdown heights (include/hsddp_touchdown.h): wb_rollout_terminal<64, true>
// (wb_knot.hpp, one wave) and wbq_rollout_terminal<QH, true> (wb_quad_term.hpp, the four lanes of a quad as a four-wide value) under the lane
// emulator, and of the terrain lookup behind k_td_terrain (touchdown.hpp).  It takes the whole emulator as term_emu.cpp does (emu.cpp: the handle, the
// ABI of include/hsddp.h, the per-step entry points; term_emu.cpp: the record and AL-parameter entry points) and adds the entry points below.
// tests/touchdown_common.py builds and binds it.
#include "term_emu.cpp"
#define TOUCHDOWN_HOST_ONLY 1
#include "touchdown.hpp"

extern "C" {
// As term_emu_terminal, with heights [batch][nph][4] by leg (null: the programs without the switch - the evaluation of term_emu_terminal).
int tdh_emu_terminal(hsddp_handle_t* h, int program, const double* eps, const hsddp_option_t* opt, int wr, const double* heights, double* out) {
    if (heights == nullptr) return term_emu_terminal(h, program, eps, opt, wr, out);
    static WbCore L;
    for (int b = 0; b < h->batch; b++) for (int pi = 0; pi < h->nph; pi++) {
        double* o = out + 4 * ((size_t)b * h->nph + pi);
        if (!term_owned(h, pi)) { o[0] = o[1] = o[2] = o[3] = NAN; continue; }
        const PhaseDev& P = h->ph[pi]; const PhaseDev* Pn = pi + 1 < h->nph ? &h->ph[pi + 1] : nullptr;
        const double* td = heights + 4 * ((size_t)b * h->nph + pi);
        if (program == 0) {
            double s4[4] = {NAN, NAN, NAN, NAN};
            SlotOut so{s4, s4 + 1, s4 + 3, s4 + 2};
            wb_rollout_terminal<64, true>(L, P, Pn, h->md, b, eps[b], opt->AL_active, so, 0, false, wr != 0, td);
            for (int q = 0; q < 4; q++) o[q] = s4[q];
        } else {
            const QuadTermOut q = wbq_rollout_terminal<QH, true>(P, Pn, h->md, b, eps[b], opt->AL_active, wr != 0, td);
            o[0] = q.cost; o[1] = q.dsq; o[2] = q.maxh; o[3] = 0.0;
        }
    }
    return 0;
}
// AL parameters of a phase's touchdown constraint as they are: sigma, lambda [batch][4] by constraint index (NaN behind nt)
int tdh_emu_get_al(hsddp_handle_t* h, int pi, double* sigma, double* lambda) {
    const PhaseDev& P = h->ph[pi];
    for (int b = 0; b < h->batch; b++) for (int i = 0; i < 4; i++) {
        sigma[4 * b + i] = i < P.nt ? P.sigma[(size_t)b * P.nt + i] : NAN; lambda[4 * b + i] = i < P.nt ? P.lambda[(size_t)b * P.nt + i] : NAN;
    }
    return P.nt;
}
// k_td_terrain's loop on the host (touchdown.hpp): foot_pos[pi] rows of 12 with ref_pb[pi] rows per problem, terminal knot hz[pi]; out [nph][batch][4]
int tdh_emu_terrain(const double* H, const int* map_of, int map_stride, int nx, int ny, int n_maps, double x0, double y0, double cx, double cy, double z_ground,
                    int nph, int batch, const double* const* foot_pos, const int* ref_pb, const int* hz, const int* on, double* out) {
    const hs::TdGrid g{H, map_of, map_stride, nx, ny, n_maps, x0, y0, cx, cy, z_ground};
    std::vector<hs::TdFootRef> r(nph);
    for (int i = 0; i < nph; i++) r[i] = hs::TdFootRef{foot_pos[i], ref_pb[i], hz[i]};
    hs::td_terrain_host(g, r.data(), on, nph, batch, out);
    return 0;
}
// the argument rules (touchdown.hpp) as the library applies them
int tdh_emu_check_set(int nph, int batch, int f32, const int* model, const int* nt, int phase, int b0, int nb, const double* heights, int src_device) {
    std::vector<hs::TdPhaseInfo> ph(nph); for (int i = 0; i < nph; i++) ph[i] = hs::TdPhaseInfo{model[i], nt[i]};
    return hs::td_check_set(hs::TdHandleInfo{nph, batch, f32}, ph.data(), phase, b0, nb, heights, src_device);
}
int tdh_emu_check_terrain(int batch, int f32, int nx, int ny, int n_maps, double x0, double y0, double cx, double cy, double z_ground, const double* H, const int* map_of, int src_device) {
    return hs::td_check_terrain(hs::TdHandleInfo{1, batch, f32}, nx, ny, n_maps, x0, y0, cx, cy, z_ground, H, map_of, src_device);
}
}
