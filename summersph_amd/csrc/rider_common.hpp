// rider_common.hpp -- the small reductions of a fixed-h step as device functions, so that each exists once and runs in two
// forms: as the stand-alone kernel it always was (pairs.hip) and as a "rider" of a persistent pair kernel
// (tiled.hip).  A rider is a workgroup behind the persistent grid of density_wt / forces_q (blockIdx.x >= the persistent
// workgroups): the dispatcher starts it on the first CU whose persistent workgroup has finished, i.e. in the partly filled
// last round of the launch, where that CU would otherwise idle until the slowest workgroup is done.  A rider reads only what
// earlier launches wrote and never waits for another workgroup (no ticket, no fence hand-over), so it is the stand-alone
// kernel minus its launch.  Block size, items per block and the order of every sum are those of the stand-alone kernels:
// the results are theirs bit for bit (tests/test_step_riders_gpu.py).
#pragma once
#include "reduce_common.hpp"

namespace sph {

constexpr int SA_BLOCK = 256;        // sink_accel_partial: threads per block (a rider workgroup of 1024 runs four blocks)
constexpr int RIDER_BS = 1024;       // threads of a rider workgroup = those of the persistent kernels

// What the riders of density_wt need beyond the kernel's own arguments (the records, the sorted order's ids and the counts are
// density_wt's too; they change hands at every grid build, these do not), in device memory (sph_ctx::d_dens_riders; rewritten
// only when a value changes): one pointer among the kernel's arguments, nothing in the pair loop's scalar registers.
struct DensRiders { const double *sink; double *sink_part; int32_t sa_blocks; };
// ... and the rider of forces_q: sink_accel_final
struct ForceRiders { const double *sink_part; double *sink; int32_t sa_blocks, ns; };

// block `blk` of `nblk` of sink_accel_partial, by the SA_BLOCK threads tid = 0 .. SA_BLOCK - 1 that share sm; a block with
// blk >= nblk only keeps the barriers (the last rider workgroup when nblk is no multiple of four)
__device__ __forceinline__ void sink_partial_block(double G, int ns, const double4 *__restrict__ drec, int64_t n,
                                                   const double *__restrict__ sink, double *__restrict__ part,
                                                   const int32_t *__restrict__ orig, int32_t n_owned, int blk, int nblk, int tid,
                                                   double (*sm)[SA_BLOCK / WAVE]) {
    const int lane = tid & 63, wv = tid >> 6;
    for (int s = 0; s < ns; s++) {
        const double sx = sink[0 * MAX_SINKS + s], sy = sink[1 * MAX_SINKS + s], sz = sink[2 * MAX_SINKS + s];
        double b0 = 0.0, b1 = 0.0, b2 = 0.0;
        if (blk < nblk) {
            for (int64_t j = (int64_t)blk * SA_BLOCK + tid; j < n; j += (int64_t)nblk * SA_BLOCK) {
                if (orig[j] >= n_owned) continue;                                       // ghosts are summed by their owners
                const double4 p = drec[j];
                const double v0 = p.x - sx, v1 = p.y - sy, v2 = p.z - sz;              // [F]:569
                const double dr = sqrt(v0 * v0 + v1 * v1 + v2 * v2);                   // [F]:570
                const double d3 = dr * dr * dr;
                b0 = b0 + (p.w * (G * v0 / d3)); b1 = b1 + (p.w * (G * v1 / d3)); b2 = b2 + (p.w * (G * v2 / d3));  // [F]:572-573
            }
        }
        b0 = wave_sum(b0); b1 = wave_sum(b1); b2 = wave_sum(b2);
        if (lane == 0) { sm[0][wv] = b0; sm[1][wv] = b1; sm[2][wv] = b2; }
        __syncthreads();
        if (tid < 3 && blk < nblk) {
            double r = 0.0;
            for (int k = 0; k < SA_BLOCK / WAVE; k++) r += sm[tid][k];
            part[((size_t)blk * MAX_SINKS + s) * 3 + tid] = r;
        }
        __syncthreads();
    }
}

// sink_accel_final for sink s, component comp, by one wave: lanes stride over the per-block partials, then a fixed-order
// wave reduction
__device__ __forceinline__ void sink_final_wave(const double *__restrict__ part, int nblocks, double *__restrict__ sink, int s,
                                                int comp, int lane) {
    double b = 0.0;
    for (int k = lane; k < nblocks; k += 64) b += part[((size_t)k * MAX_SINKS + s) * 3 + comp];
    b = wave_sum(b);
    if (lane == 0) sink[(7 + comp) * MAX_SINKS + s] = b;
}

// The riders of a density_wt launch: ceil(sa_blocks / 4) workgroups, each four blocks of sink_accel_partial side by side with
// their own twelve doubles of LDS.  rider = blockIdx.x - persistent workgroups; lds = the launch's dynamic LDS (a rider declares
// no static LDS: nothing may shift the tile).  Workgroup-uniform throughout.
__device__ __forceinline__ void density_riders(const DensRiders *__restrict__ ra, int rider, double *lds, double G, int ns,
                                               const double4 *__restrict__ drec, int64_t n, const int32_t *__restrict__ orig,
                                               int32_t n_owned) {
    const int sub = threadIdx.x / SA_BLOCK;
    auto sm = reinterpret_cast<double (*)[SA_BLOCK / WAVE]>(lds + sub * 3 * (SA_BLOCK / WAVE));
    sink_partial_block(G, ns, drec, n, ra->sink, ra->sink_part, orig, n_owned, rider * (RIDER_BS / SA_BLOCK) + sub, ra->sa_blocks,
                       (int)threadIdx.x % SA_BLOCK, sm);
}

// The rider of a forces_q launch: sink_accel_final of every sink, three waves a sink (five sinks per pass of the sixteen waves)
__device__ __forceinline__ void forces_rider(const ForceRiders *__restrict__ ra) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = wv / 3; wv < 15 && s < ra->ns; s += 5) sink_final_wave(ra->sink_part, ra->sa_blocks, ra->sink, s, wv % 3, lane);
}

}  // namespace sph
