// TEST-ONLY: a stand-alone program around the host side of the plant table (cafe-mpc_amd/csrc/plant_host.hpp: the validation hsddp_plant_set runs and the
// packing of what it uploads), for -fsanitize=address,undefined.  tests/test_plant_host.py compiles and runs it; it checks every refusal of
// include/hsddp_plant.h on heap arrays of exactly the sizes the calls may read, and prints "plant_table_asan: clean" when all of them answered as expected.
#include <cstdio>
#include <limits>
#include <vector>
#include "plant_host.hpp"

using namespace hs;

static int failures = 0;
static void expect(bool got, bool want, const char* what) {
    if (got != want) { std::printf("plant_table_asan: %s: got %d, want %d\n", what, (int)got, (int)want); failures++; }
}

int main() {
    double nominal[PLANT_ROW] = {3.3, 0, 0, 0, 0.011253, 0, 0, 0.036203, 0, 0.042673};      // ... twelve link scales and twelve gains of 1, twelve dampings of 0
    for (int i = 10; i < 34; i++) nominal[i] = 1.0;
    const int n = 3; const size_t total = 20;
    std::vector<double> P((size_t)n * PLANT_ROW);
    for (int p = 0; p < n; p++) for (int i = 0; i < PLANT_ROW; i++) P[(size_t)p * PLANT_ROW + i] = nominal[i];
    P[PLANT_ROW] = 4.3; P[PLANT_ROW + 1] = 0.0116; P[2 * PLANT_ROW + 10] = 0.8; P[2 * PLANT_ROW + 22] = 0.9; P[2 * PLANT_ROW + 45] = 0.01;
    std::vector<int> of(total);
    for (size_t i = 0; i < total; i++) of[i] = (int)(i % n);
    expect(plant_table_ok(n, P.data(), of.data(), total), true, "a good table");
    expect(plant_table_ok(n, P.data(), nullptr, total), true, "a good table without an index");
    expect(plant_table_ok(n, nullptr, of.data(), total), false, "a null table");
    expect(plant_table_ok(0, P.data(), of.data(), total), false, "no rows");
    expect(plant_table_ok(PLANT_MAX + 1, P.data(), of.data(), total), false, "too many rows");      // (refused before a row is read)
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct Bad { int at; double v; const char* what; };
    const Bad bad[] = {{0, 0.0, "mass 0"}, {0, -1.0, "mass < 0"}, {PLANT_ROW + 2, nan, "a NaN CoM"}, {2 * PLANT_ROW + 45, inf, "an infinite damping"},
                       {4, 0.0, "Ixx 0"}, {5, 0.03, "second minor < 0"}, {9, -0.01, "Izz < 0"}, {2 * PLANT_ROW + 8, 0.05, "determinant < 0"},
                       {PLANT_ROW + 13, 0.0, "link_scale 0"}, {2 * PLANT_ROW + 21, -0.5, "link_scale < 0"}, {34, -1e-9, "damping < 0"}};
    for (const Bad& b : bad) {
        std::vector<double> Q = P;      // a fresh heap copy of the exact size
        Q[(size_t)b.at] = b.v;
        expect(plant_table_ok(n, Q.data(), of.data(), total), false, b.what);
    }
    {
        std::vector<double> Q = P; Q[22] = -2.0; Q[23] = 0.0;      // any finite gain is a plant
        expect(plant_table_ok(n, Q.data(), of.data(), total), true, "a negative and a zero gain");
    }
    for (int v : {-1, n}) {
        std::vector<int> o2 = of; o2[total - 1] = v;
        expect(plant_table_ok(n, P.data(), o2.data(), total), false, "an index outside the table");
    }
    std::vector<double> rows; std::vector<int> idx;
    plant_table_pack(n, P.data(), of.data(), total, rows, idx);
    expect(rows == P && idx == of, true, "the packed table");
    plant_table_pack(1, P.data(), nullptr, total, rows, idx);
    expect(rows.size() == (size_t)PLANT_ROW && idx.size() == total && idx[total - 1] == 0, true, "the packed table without an index");
    if (failures == 0) std::printf("plant_table_asan: clean\n");
    return failures == 0 ? 0 : 1;
}
