// Stand-alone walk over the pure host part of per-problem cost-weight scales (cafe-mpc_amd/csrc/weights.hpp): the argument rules of
// hsddp_weights_set / hsddp_weights_get and k_pack_weights' loop, on exactly-sized heap buffers so that AddressSanitizer sees any read or write
// beyond a range.  tests/test_weights_host.py builds it with -fsanitize=address,undefined and runs it on its own.  Prints "ok <checks>".
#define WEIGHTS_HOST_ONLY 1
#include "weights.hpp"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int checks = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); return 1; } checks++; } while (0)

int main() {
    using namespace hs;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int batch : {1, 5, 17}) {
        const WsHandleInfo H{batch, 0}, H32{batch, 1};
        for (int b0 = -1; b0 <= batch; b0++) for (int nb = -1; nb <= batch + 1; nb++) {
            const bool in = nb > 0 && b0 >= 0 && b0 + nb <= batch;
            std::vector<double> rows((size_t)(nb > 0 ? nb : 0) * WSP_ROW, 1.5);      // exactly the rows the call may read
            CHECK(ws_check_range(H, b0, nb) == (in ? WS_OK : WS_EINVAL));
            CHECK(ws_check_range(H32, b0, nb) == (in ? WS_ENOTSUP : WS_EINVAL));
            CHECK(ws_check_set(H, b0, nb, nullptr, 0) == WS_EINVAL);
            CHECK(ws_check_set(H, b0, nb, rows.data(), 0) == (in ? WS_OK : WS_EINVAL));
            CHECK(ws_check_set(H, b0, nb, rows.data(), 1) == (in ? WS_OK : WS_EINVAL));
            if (!in) continue;
            for (int e : {0, 35, 36, 47, 48, 83}) for (double bad : {nan, inf, -inf, -1.0, 0.0}) {
                std::vector<double> r2 = rows; r2[(size_t)(nb - 1) * WSP_ROW + e] = bad;
                const bool sr = e >= WSP_R && e < WSP_QF, fine = bad == 0.0 && !sr;      // a zero is a weight switched off: allowed for sq, sqf, not for sr
                CHECK(ws_check_set(H, b0, nb, r2.data(), 0) == (fine ? WS_OK : WS_EINVAL));
                CHECK(ws_check_set(H, b0, nb, r2.data(), 1) == WS_OK);      // a device source is not read
            }
            // the packing loop: first call (whole table, 1.0 outside the range), then the range alone on a table of sentinels
            std::vector<double> table((size_t)batch * WSP_ROW, -7.0), src((size_t)nb * WSP_ROW);
            for (size_t i = 0; i < src.size(); i++) src[i] = 0.25 + 0.001 * (double)i;
            ws_pack_host(WsPack{table.data(), src.data(), b0, nb, 0, batch});
            for (int b = 0; b < batch; b++) for (int e = 0; e < WSP_ROW; e++) {
                const double want = (b >= b0 && b < b0 + nb) ? src[(size_t)(b - b0) * WSP_ROW + e] : 1.0;
                CHECK(table[(size_t)b * WSP_ROW + e] == want);
            }
            std::vector<double> t2((size_t)batch * WSP_ROW, -7.0);
            ws_pack_host(WsPack{t2.data(), src.data(), b0, nb, b0, nb});
            for (int b = 0; b < batch; b++) for (int e = 0; e < WSP_ROW; e++) {
                const double want = (b >= b0 && b < b0 + nb) ? src[(size_t)(b - b0) * WSP_ROW + e] : -7.0;
                CHECK(t2[(size_t)b * WSP_ROW + e] == want);
            }
        }
    }
    std::printf("ok %d\n", checks);
    return 0;
}
