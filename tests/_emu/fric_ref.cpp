// TEST-ONLY: the CPU oracle plus ONE function for Coulomb friction (include/hsddp_friction.h).  fric_ref_dynamics is wb_forward / wb_dynamics of
// oracle/wbm.hpp restated with a row mask per foot and an added foot force: it takes wb_terms on the attached feet, removes the x and y rows of J and
// gamma of every foot flagged as sliding, adds J_f^T f_t of those feet to tau - h (with the rows it is about to remove), and solves as wb_forward does,
// statement for statement, so that a call without a sliding foot reproduces oracle_wb_dynamics bit for bit.  tests/fric_common.py builds it into a
// temporary directory with the oracle's own flags; the oracle the solves run on is never touched.
#include "oracle_api.cpp"

// contact [4]: the attached feet; slide [4]: 1 for an attached foot held by its z row alone; ft [4][2]: the tangential force on such a foot (world x, y).
// xnext [36]: forward Euler with dt; y [12]: the multipliers by leg (a sliding foot: 0, 0, lambda_z); wt [4][2]: the tangential velocity of every foot point.
extern "C" void fric_ref_dynamics(const double* x, const double* u, const int* contact, const int* slide, const double* ft, double psi_dyn, double psi_kin, double alpha, double dt,
                                  double* xnext, double* y, double* wt) {
    using namespace orc;
    WbParams P; P.psi_dyn = psi_dyn; P.psi_kin = psi_kin; P.bg_alpha = alpha;
    const double* q = x; const double* v = x + NQ;
    double tau[NQ] = {0}; for (int i = 0; i < NU; i++) tau[6 + i] = u[i];
    WbKKT K; set_contacts(K, contact);
    wb_terms(P, q, v, K);
    for (int l = 0; l < 4; l++) { wt[2 * l] = K.foot_vel[l].x; wt[2 * l + 1] = K.foot_vel[l].y; }
    double L[NQ * NQ]; std::memcpy(L, K.M, sizeof(L)); chol(L, NQ);
    double r[NQ];
    for (int i = 0; i < NQ; i++) r[i] = tau[i] - K.h[i];
    for (int c = 0; c < K.nc; c++) if (slide[K.feet[c]]) for (int i = 0; i < NQ; i++) r[i] += K.J[(3 * c + 0) * NQ + i] * ft[2 * K.feet[c]] + K.J[(3 * c + 1) * NQ + i] * ft[2 * K.feet[c] + 1];
    // the rows that stay: all three of a sticking foot, z of a sliding one
    int m = 0, leg[12], dir[12]; double J[12 * NQ], gamma[12];
    for (int c = 0; c < K.nc; c++) for (int d = 0; d < 3; d++) {
        if (slide[K.feet[c]] && d < 2) continue;
        for (int i = 0; i < NQ; i++) J[m * NQ + i] = K.J[(3 * c + d) * NQ + i];
        gamma[m] = K.gamma[3 * c + d]; leg[m] = K.feet[c]; dir[m] = d; m++;
    }
    double a0[NQ]; std::memcpy(a0, r, sizeof(r)); chol_solve(L, NQ, a0);
    double qdd[NQ];
    for (int i = 0; i < 12; i++) y[i] = 0.0;
    if (m > 0) {
        double MiJt[NQ * 12], G[12 * 12], rhs[12];
        for (int c = 0; c < m; c++) {
            double col[NQ]; for (int i = 0; i < NQ; i++) col[i] = J[c * NQ + i];
            chol_solve(L, NQ, col);
            for (int i = 0; i < NQ; i++) MiJt[i * 12 + c] = col[i];
        }
        for (int a = 0; a < m; a++) for (int b = 0; b < m; b++) {
            double s = 0; for (int i = 0; i < NQ; i++) s += J[a * NQ + i] * MiJt[i * 12 + b];
            G[a * m + b] = s + (a == b ? 1e-12 : 0.0);
        }
        chol(G, m);
        for (int a = 0; a < m; a++) { double s = 0; for (int i = 0; i < NQ; i++) s += J[a * NQ + i] * a0[i]; rhs[a] = -s - gamma[a]; }
        chol_solve(G, m, rhs);
        for (int i = 0; i < NQ; i++) { double s = r[i]; for (int a = 0; a < m; a++) s += J[a * NQ + i] * rhs[a]; r[i] = s; }
        chol_solve(L, NQ, r);
        std::memcpy(qdd, r, sizeof(r));
        for (int a = 0; a < m; a++) y[3 * leg[a] + dir[a]] = rhs[a];
    } else std::memcpy(qdd, a0, sizeof(a0));
    for (int i = 0; i < NQ; i++) { xnext[i] = q[i] + v[i] * dt; xnext[NQ + i] = v[i] + qdd[i] * dt; }
}
