// Stand-alone walk over the pure host part of per-problem constraint limits (cafe-mpc_amd/csrc/limits.hpp): the argument rules of hsddp_limits_set /
// hsddp_limits_get / hsddp_episode_plan_friction and the loops of k_pack_limits and k_lim_mu, on exactly-sized heap buffers so that
// AddressSanitizer sees any read or write beyond a range.  tests/test_limits_host.py builds it with -fsanitize=address,undefined and runs it on its
// own.  Prints "ok <checks>".
#define LIMITS_HOST_ONLY 1
#include "limits.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int checks = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); return 1; } checks++; } while (0)
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

int main() {
    using namespace hs;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double good[LMP_ROW] = {12.0, -0.3, -1.2, 1.8, 0.3, -0.8, 2.2, 0.1, 0.4, -3.0, 3.0, nan};
    CHECK(lim_check_kappa(1.0) == LIM_OK && lim_check_kappa(0.25) == LIM_OK);
    for (double k : {0.0, -0.5, 1.0000001, nan, inf}) CHECK(lim_check_kappa(k) == LIM_EINVAL);
    for (int batch : {1, 5, 17}) for (int nph : {1, 3}) {
        const LimHandleInfo H{batch, nph, 0}, H32{batch, nph, 1};
        for (int ph : {-1, 0, nph - 1, nph}) CHECK(lim_check_get(H, ph, 0, batch) == ((ph >= 0 && ph < nph) ? LIM_OK : LIM_EINVAL));
        CHECK(lim_check_get(H32, 0, 0, batch) == LIM_ENOTSUP);
        for (int b0 = -1; b0 <= batch; b0++) for (int nb = -1; nb <= batch + 1; nb++) {
            const bool in = nb > 0 && b0 >= 0 && b0 + nb <= batch;
            std::vector<double> rows((size_t)(nb > 0 ? nb : 0) * LMP_ROW);      // exactly the rows the call may read
            for (size_t i = 0; i < rows.size(); i++) rows[i] = good[i % LMP_ROW];
            CHECK(lim_check_range(H, b0, nb) == (in ? LIM_OK : LIM_EINVAL));
            CHECK(lim_check_range(H32, b0, nb) == (in ? LIM_ENOTSUP : LIM_EINVAL));
            CHECK(lim_check_set(H, b0, nb, nullptr, 0) == LIM_EINVAL);
            CHECK(lim_check_set(H, b0, nb, rows.data(), 0) == (in ? LIM_OK : LIM_EINVAL));
            CHECK(lim_check_set(H, b0, nb, rows.data(), 1) == (in ? LIM_OK : LIM_EINVAL));
            if (!in) continue;
            for (int e = 0; e < LMP_ROW; e++) {      // every entry: NaN is "unset", an infinity is refused (pad: anything goes)
                for (double v : {nan, inf, -inf}) {
                    std::vector<double> r2 = rows; r2[(size_t)(nb - 1) * LMP_ROW + e] = v;
                    CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == ((v != v || e == LMP_PAD) ? LIM_OK : LIM_EINVAL));
                    CHECK(lim_check_set(H, b0, nb, r2.data(), 1) == LIM_OK);      // a device source is not read
                }
            }
            for (int e : {LMP_TORQUE, LMP_MU}) for (double v : {0.0, -1.0}) { std::vector<double> r2 = rows; r2[e] = v; CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == LIM_EINVAL); }
            for (int j = 0; j < 3; j++) {
                std::vector<double> r2 = rows; r2[LMP_JLB + j] = r2[LMP_JUB + j]; CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == LIM_EINVAL);
                r2[LMP_JUB + j] = nan; CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == LIM_OK);      // only one of the pair given: nothing to compare
            }
            { std::vector<double> r2 = rows; r2[LMP_JSLB] = 4.0; CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == LIM_EINVAL); r2[LMP_JSUB] = nan; CHECK(lim_check_set(H, b0, nb, r2.data(), 0) == LIM_OK); }
            // the packing loop: first call (whole table, NaN outside the range), a later call on tables of sentinels, then a resolve against new descriptors
            std::vector<double> user((size_t)batch * LMP_ROW, -7.0), res((size_t)nph * batch * LMP_ROW, -7.0), desc((size_t)nph * LMP_ROW), src((size_t)nb * LMP_ROW);
            for (size_t i = 0; i < desc.size(); i++) desc[i] = 100.0 + (double)i;
            for (size_t i = 0; i < src.size(); i++) src[i] = (i % 5 == 0) ? nan : 0.25 + 0.001 * (double)i;
            lim_pack_host(LimPack{user.data(), res.data(), src.data(), desc.data(), batch, nph, b0, nb, 0, batch, LIM_PACK_FIRST});
            for (int b = 0; b < batch; b++) for (int e = 0; e < LMP_ROW; e++) {
                const double u = (b >= b0 && b < b0 + nb) ? src[(size_t)(b - b0) * LMP_ROW + e] : nan;
                CHECK(same(user[(size_t)b * LMP_ROW + e], u));
                for (int p = 0; p < nph; p++) CHECK(same(res[((size_t)p * batch + b) * LMP_ROW + e], u != u ? desc[(size_t)p * LMP_ROW + e] : u));
            }
            std::vector<double> u2((size_t)batch * LMP_ROW, -7.0), r2((size_t)nph * batch * LMP_ROW, -7.0);
            lim_pack_host(LimPack{u2.data(), r2.data(), src.data(), desc.data(), batch, nph, b0, nb, b0, nb, LIM_PACK_RANGE});
            for (int b = 0; b < batch; b++) for (int e = 0; e < LMP_ROW; e++) {
                const bool inr = b >= b0 && b < b0 + nb; const double u = inr ? src[(size_t)(b - b0) * LMP_ROW + e] : -7.0;
                CHECK(same(u2[(size_t)b * LMP_ROW + e], u));
                for (int p = 0; p < nph; p++) CHECK(same(r2[((size_t)p * batch + b) * LMP_ROW + e], !inr ? -7.0 : u != u ? desc[(size_t)p * LMP_ROW + e] : u));
            }
            for (size_t i = 0; i < desc.size(); i++) desc[i] = 500.0 - (double)i;
            lim_pack_host(LimPack{user.data(), res.data(), nullptr, desc.data(), batch, nph, 0, 0, 0, batch, LIM_PACK_RESOLVE});
            for (int b = 0; b < batch; b++) for (int e = 0; e < LMP_ROW; e++) for (int p = 0; p < nph; p++) {
                const double u = user[(size_t)b * LMP_ROW + e];
                CHECK(same(res[((size_t)p * batch + b) * LMP_ROW + e], u != u ? desc[(size_t)p * LMP_ROW + e] : u));
            }
            // the friction fill: only the mu column moves
            for (int stride : {1, 3}) {
                std::vector<double> mu_tab = {0.6, 0.5, 0.25, 0.2, 0.3, 0.3}; std::vector<int> mu_of((size_t)batch * stride);
                for (size_t i = 0; i < mu_of.size(); i++) mu_of[i] = (int)(i % 3);
                std::vector<double> uf = user, rf = res;
                lim_mu_host(LimMu{uf.data(), rf.data(), mu_tab.data(), mu_of.data(), stride, batch, nph, 0.7});
                for (int b = 0; b < batch; b++) for (int e = 0; e < LMP_ROW; e++) {
                    const double m = 0.7 * mu_tab[2 * (size_t)mu_of[(size_t)b * stride]];
                    CHECK(same(uf[(size_t)b * LMP_ROW + e], e == LMP_MU ? m : user[(size_t)b * LMP_ROW + e]));
                    for (int p = 0; p < nph; p++) CHECK(same(rf[((size_t)p * batch + b) * LMP_ROW + e], e == LMP_MU ? m : res[((size_t)p * batch + b) * LMP_ROW + e]));
                }
            }
        }
    }
    std::printf("ok %d\n", checks);
    return 0;
}
