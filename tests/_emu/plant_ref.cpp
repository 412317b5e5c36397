// TEST-ONLY: the CPU oracle with link constants a test can vary per sample (include/hsddp_plant.h).  The oracle's model constants sit in a function-local
// static that is not declared const (orc::wbc(), oracle/wbm.hpp); this shim takes the whole oracle in and adds plant_ref_set, which resets those
// constants to a fresh WbConst, overwrites the trunk (link 5) and scales the mass and CoM inertia of the twelve leg links (links 6 .. 17, leg-major).
// CoMs and geometry stay.  The nominal arguments reproduce the oracle bit for bit.  tests/plant_common.py builds it into a temporary directory with the
// oracle's own flags; the oracle's solves are OpenMP-parallel, so the constants are set only between calls.
#include "oracle_api.cpp"

extern "C" void plant_ref_set(const double* trunk /* [10] mass | CoM | inertia about the CoM */, const double* scale /* [12] */) {
    orc::WbConst& c = const_cast<orc::WbConst&>(orc::wbc());
    c = orc::WbConst();
    c.link[5].m = trunk[0];
    for (int i = 0; i < 3; i++) c.link[5].c[i] = trunk[1 + i];
    for (int i = 0; i < 6; i++) c.link[5].I[i] = trunk[4 + i];
    for (int j = 0; j < 12; j++) {
        c.link[6 + j].m *= scale[j];
        for (int i = 0; i < 6; i++) c.link[6 + j].I[i] *= scale[j];
    }
}
