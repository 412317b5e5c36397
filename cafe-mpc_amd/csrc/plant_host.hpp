// Host side of the plant table (include/hsddp_plant.h): the validation of a table and the packing of what goes to the device.  Plain C++ without a
// HIP header, so that hsddp_plant_set, the host build of the tests (tests/_emu/plant_emu.cpp) and the stand-alone sanitizer program
// (tests/cpp/plant_table_asan.cpp) share ONE copy of the refusals.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace hs {

constexpr int PLANT_ROW = 46, PLANT_MAX = 65536;

// true if the table is one hsddp_plant_set accepts: P [n_plants][PLANT_ROW], plant_of [total] or null
inline bool plant_table_ok(int n_plants, const double* P, const int* plant_of, size_t total) {
    if (!P || n_plants < 1 || n_plants > PLANT_MAX) return false;
    for (int p = 0; p < n_plants; p++) {
        const double* r = P + (size_t)p * PLANT_ROW;
        for (int i = 0; i < PLANT_ROW; i++) if (!std::isfinite(r[i])) return false;
        if (!(r[0] > 0.0)) return false;
        const double xx = r[4], xy = r[5], xz = r[6], yy = r[7], yz = r[8], zz = r[9];      // leading minors of the trunk inertia
        if (!(xx > 0.0) || !(xx * yy - xy * xy > 0.0)) return false;
        if (!(xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz) > 0.0)) return false;
        for (int j = 0; j < 12; j++) if (!(r[10 + j] > 0.0) || r[34 + j] < 0.0) return false;
    }
    if (plant_of) for (size_t i = 0; i < total; i++) if (plant_of[i] < 0 || plant_of[i] >= n_plants) return false;
    return true;
}

// what the device gets: the rows as they are and an index per sample (row 0 where plant_of is null)
inline void plant_table_pack(int n_plants, const double* P, const int* plant_of, size_t total, std::vector<double>& rows, std::vector<int>& idx) {
    rows.assign(P, P + (size_t)n_plants * PLANT_ROW);
    if (plant_of) idx.assign(plant_of, plant_of + total);
    else idx.assign(total, 0);
}

}  // namespace hs
