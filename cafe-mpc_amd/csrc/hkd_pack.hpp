// HKD-MPC command export (include/hsddp_hkd.h): k_pack_hkd packs hkd_command_lcmt rows for a range of problems in one launch.
//
//   grid (nb), 256 threads: one workgroup per problem.  The row is assembled in LDS and then written out with consecutive lanes on consecutive
//   words (8-byte stores when the destination allows: a row is 1954 words, so every row starts on an 8-byte boundary of an 8-byte aligned
//   buffer).  The 12 x 12 feedback block of a knot is read column by column (12 contiguous doubles at a stride of 24: K is column-major
//   24 x 24) and transposed into the message's row-major order in LDS, so no lane gathers at a stride of 24.  Doubles (mpc_times, statusTimes)
//   go out as two words, low word first.
//   The step -> (phase, k) walk and the foothold phase of every leg are the same for the whole batch (contacts are shared): the host derives
//   them once per call (HkdMap), the kernel only reads them.
#pragma once

namespace hs {

constexpr int HKD_W = HSDDP_HKD_CMD_WORDS;
constexpr int HKD_MAXS = HSDDP_HKD_MAX_STEPS;
struct HkdMap { int ph[HKD_MAXS], k[HKD_MAXS], fh[4]; };      // knot s of the message -> (phase, knot); leg l -> phase of its next foothold or -1

// mpc_time + k * dt rounded as written: a product, then a sum (the host statement of the row is not fused into a multiply-add either)
__device__ inline double hkd_time(double t0, int k, double dt) {
#pragma clang fp contract(off)
    const double p = (double)k * dt;
    return t0 + p;
}

// words of one double, low word first (little-endian hosts: what a memcpy of the struct holds)
__device__ inline void hkd_put_double(unsigned int* row, int w, double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    row[w] = (unsigned int)u; row[w + 1] = (unsigned int)(u >> 32);
}

__global__ void __launch_bounds__(256) k_pack_hkd(const PhaseDev* ph, const HkdMap* map, int b0, int n_steps, double t0, double dt,
                                                  const double* status, const float* pf_in, float solve_ms, unsigned int* out, int vec2) {
    __shared__ uint2 rowv[(HKD_W + 1) / 2];
    __shared__ const HS_GLOBAL double *sU[HKD_MAXS], *sX[HKD_MAXS], *sK[HKD_MAXS], *sF[4];
    __shared__ int sC[HKD_MAXS][4], sP[HKD_MAXS];
    unsigned int* row = reinterpret_cast<unsigned int*>(rowv);
    const int i = blockIdx.x, b = b0 + i, t = threadIdx.x;
    // per-knot base pointers of this problem (and the knot-0 state of every foothold phase)
    if (t < HKD_MAXS) {
        if (t < n_steps) {
            const PhaseDev& P = ph[map->ph[t]]; const int k = map->k[t]; const size_t kk = (size_t)b * P.h + k;
            sU[t] = P.Ubar + kk * 24; sX[t] = P.Xbar + ((size_t)b * (P.h + 1) + k) * 24; sK[t] = P.K + kk * 576; sP[t] = map->ph[t];
            for (int l = 0; l < 4; l++) sC[t][l] = P.contact[l];
        } else {
            sU[t] = sX[t] = sK[t] = nullptr; sP[t] = -1; for (int l = 0; l < 4; l++) sC[t][l] = 0;
        }
    } else if (t >= 64 && t < 68) {
        const int l = t - 64, f = map->fh[l];
        sF[l] = f >= 0 ? ph[f].Xbar + (size_t)b * (ph[f].h + 1) * 24 + 12 + 3 * l : nullptr;
    }
    __syncthreads();
    // feedback[s][m][n] = K_s[n * 24 + m]: lane e reads column n, row m (12 contiguous doubles per column)
    for (int e = t; e < HKD_MAXS * 144; e += blockDim.x) {
        const int s = e / 144, r = e - s * 144, n = r / 12, m = r - n * 12;
        const float v = s < n_steps ? (float)sK[s][n * 24 + m] : 0.f;
        row[HSDDP_HKD_OFF_FEEDBACK + s * 144 + m * 12 + n] = __float_as_uint(v);
    }
    for (int e = t; e < HKD_MAXS * 24; e += blockDim.x) {
        const int s = e / 24, j = e - s * 24;
        row[HSDDP_HKD_OFF_CONTROLS + e] = __float_as_uint(s < n_steps ? (float)sU[s][j] : 0.f);
    }
    for (int e = t; e < HKD_MAXS * 12; e += blockDim.x) {
        const int s = e / 12, j = e - s * 12;
        row[HSDDP_HKD_OFF_BODY_STATE + e] = __float_as_uint(s < n_steps ? (float)sX[s][j] : 0.f);
    }
    // the small fields: N_mpcsteps, mpc_times, contacts, statusTimes, foot_placement, solve_time (one lane per word or per double)
    constexpr int NT = 1 + HKD_MAXS + 4 * HKD_MAXS + 4 * HKD_MAXS + 12 + 1;
    for (int e = t; e < NT; e += blockDim.x) {
        int q = e;
        if (q == 0) { row[HSDDP_HKD_OFF_N_MPCSTEPS] = (unsigned int)n_steps; continue; }
        q -= 1;
        if (q < HKD_MAXS) {      // mpc_time + k * dt in fp64
            hkd_put_double(row, HSDDP_HKD_OFF_MPC_TIMES + 2 * q, q < n_steps ? hkd_time(t0, q, dt) : 0.0); continue;
        }
        q -= HKD_MAXS;
        if (q < 4 * HKD_MAXS) { row[HSDDP_HKD_OFF_CONTACTS + q] = (unsigned int)sC[q >> 2][q & 3]; continue; }
        q -= 4 * HKD_MAXS;
        if (q < 4 * HKD_MAXS) {
            const int s = q >> 2;
            hkd_put_double(row, HSDDP_HKD_OFF_STATUS_TIMES + 2 * q, (s < n_steps && status) ? status[sP[s] * 4 + (q & 3)] : 0.0); continue;
        }
        q -= 4 * HKD_MAXS;
        if (q < 12) {
            const int l = q / 3;
            const float v = sF[l] ? (float)sF[l][q - 3 * l] : (pf_in ? pf_in[(size_t)i * 12 + q] : 0.f);
            row[HSDDP_HKD_OFF_FOOT_PLACEMENT + q] = __float_as_uint(v); continue;
        }
        row[HSDDP_HKD_OFF_SOLVE_TIME] = __float_as_uint(solve_ms);
    }
    __syncthreads();
    unsigned int* dst = out + (size_t)i * HKD_W;
    if (vec2) {
        uint2* d2 = reinterpret_cast<uint2*>(dst);
        for (int q = t; q < HKD_W / 2; q += blockDim.x) d2[q] = rowv[q];
    } else {
        for (int q = t; q < HKD_W; q += blockDim.x) dst[q] = row[q];
    }
}

}  // namespace hs
