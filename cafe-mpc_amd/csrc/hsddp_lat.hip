// The policy-latency kernel of the MPC episodes of libhsddp_hip.so (include/hsddp_latency.h; the program is epi_latency of episode.hpp) and its
// launcher.  The Makefile compiles this file on its own (-DHS_LAT_SEPARATE for hsddp_hip.hip); hsddp_hip.hip includes it when it is built without that
// switch (a one-command build of the library).  A translation unit of its own for the reason given in hsddp_sub.hip: the code object of hsddp_hip.hip
// keeps every kernel where it is, and `make resources` lists the kernels it listed.
#ifdef HS_LAT_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#define HS_SIM_WALK_ONLY 1
#define HS_EPISODE_BODIES_ONLY 1
#include "episode.hpp"
#endif

namespace hs {

// grid = min(B (n_exec + D), LAT_MAX_WAVES) waves of 64 lanes; wave w takes the (problem, step) pairs w, w + grid, ... - step fastest, so that
// neighbouring waves read neighbouring knots of one problem.  A streaming copy: no LDS, no scratch, no atomics.
__global__ void __launch_bounds__(64) k_episode_latency(const PhaseDev* ph_, EpiLatArgs a) {
    const int L = a.n_exec + a.D, n = a.B * L;
    for (int r = (int)blockIdx.x; r < n; r += (int)gridDim.x) epi_latency<EpiWaveD>((PhaseC*)ph_, a, r / L, r % L);
}

// (leaves the runtime's error state alone, as the launchers of the walks do: the caller's hipGetLastError reports a failed launch)
void epi_latency_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const EpiLatArgs& a) {
    hipLaunchKernelGGL(k_episode_latency, dim3(grid), dim3(64), 0, stream, ph, a);
}

}  // namespace hs
