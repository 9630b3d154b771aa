// energy_terms.hpp -- the per-particle terms of sph_energy's sums and its sink part (include/summersph.h, "Sums"), shared by
// energy.hip and history.hip so that both form every term with the same arithmetic in the same order.
#pragma once
#include "reduce_common.hpp"

// the arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

constexpr int ENERGY_NG = 15;                          // gas sums
constexpr int ENERGY_NK = SPH_ENERGY_NSUM - ENERGY_NG; // sink sums

// Phi_sink = -sum_s G M_s / |r - R_s| in sink order, unsoftened; massless sinks add 0
__device__ __forceinline__ double phi_sink(double x, double y, double z, const double *__restrict__ sink, int ns, double G) {
    double ps = 0.0;
    for (int s = 0; s < ns; s++) {
        const double sm = sink[6 * MAX_SINKS + s];
        if (sm == 0.0) continue;
        const double dx = x - sink[s], dy = y - sink[MAX_SINKS + s], dz = z - sink[2 * MAX_SINKS + s];
        ps = ps - (G * sm) / sqrt((dx * dx + dy * dy) + dz * dz);
    }
    return ps;
}

// the 15 gas terms of one particle (pg = Phi_self, ps = Phi_sink)
__device__ __forceinline__ void gas_terms(double x, double y, double z, double vx, double vy, double vz, double u, double m,
                                          double pg, double ps, double (&q)[ENERGY_NG]) {
    q[0] = 1.0;
    q[1] = m;
    q[2] = m * x; q[3] = m * y; q[4] = m * z;
    q[5] = m * vx; q[6] = m * vy; q[7] = m * vz;
    q[8] = m * (y * vz - z * vy); q[9] = m * (z * vx - x * vz); q[10] = m * (x * vy - y * vx);
    q[11] = (0.5 * m) * ((vx * vx + vy * vy) + vz * vz);
    q[12] = m * u;
    q[13] = (0.5 * m) * pg;
    q[14] = m * ps;
}

// the sink part, by one whole wavefront (rank 0 only; lane s: sink s, and its pair terms with the sinks t > s in t order,
// then the butterfly): every lane ends with sk[0..13) = sums[15..28)
__device__ __forceinline__ void sink_sums(int lane, const double *__restrict__ sink, int ns, int rank0, double G,
                                          double (&sk)[ENERGY_NK]) {
#pragma unroll
    for (int s = 0; s < ENERGY_NK; s++) sk[s] = 0.0;
    if (rank0 && lane < ns) {
        const double x = sink[lane], y = sink[MAX_SINKS + lane], z = sink[2 * MAX_SINKS + lane];
        const double vx = sink[3 * MAX_SINKS + lane], vy = sink[4 * MAX_SINKS + lane], vz = sink[5 * MAX_SINKS + lane];
        const double m = sink[6 * MAX_SINKS + lane];
        double w = 0.0;
        for (int t = lane + 1; t < ns; t++) {
            const double mt = sink[6 * MAX_SINKS + t];
            const double mm = m * mt;
            if (mm == 0.0) continue;
            const double dx = x - sink[t], dy = y - sink[MAX_SINKS + t], dz = z - sink[2 * MAX_SINKS + t];
            w = w - (G * mm) / sqrt((dx * dx + dy * dy) + dz * dz);
        }
        const double q[ENERGY_NK] = {1.0,
                                     m,
                                     m * x, m * y, m * z,
                                     m * vx, m * vy, m * vz,
                                     m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx),
                                     (0.5 * m) * ((vx * vx + vy * vy) + vz * vz),
                                     w};
#pragma unroll
        for (int s = 0; s < ENERGY_NK; s++) sk[s] = q[s];
    }
#pragma unroll
    for (int s = 0; s < ENERGY_NK; s++) sk[s] = wave_sum(sk[s]);
}

}  // namespace sph
