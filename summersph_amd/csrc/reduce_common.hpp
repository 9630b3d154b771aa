// reduce_common.hpp -- the wavefront reductions and the "piece" shape of the order-free sums (profile.hip, energy.hip,
// groups.hip): a run of sorted positions is cut into pieces of PIECE positions from its own start, one wavefront reduces
// each piece (lane l adds positions l, l + 64, ... in turn, then the butterfly) and a second kernel adds a run's pieces in
// the same shape.  A sum's shape then depends on its run's start and length alone, never on the launch.
// Also the min / max / count statistics of the image passes' selections (render.hip, cube.hip, transfer.hip).
#pragma once
#include "sph_internal.hpp"

namespace sph {

// xor butterflies over the 64 lanes: every lane ends with the same result
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t bad) {
    for (int o = 32; o > 0; o >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    return bad;
}

// The image passes' selection statistics (render.hip, cube.hip, transfer.hip): N values of which the first NMIN are
// minima, the next NMAX maxima and the rest counts (sums of small integers).  All three are exact in any order, so the
// values do not depend on the launch.
template <int NMIN, int NMAX>
__device__ __forceinline__ double stat_identity(int k) { return k < NMIN ? INFINITY : (k < NMIN + NMAX ? -INFINITY : 0.0); }
template <int NMIN, int NMAX>
__device__ __forceinline__ double stat_join(int k, double a, double b) {
    return k < NMIN ? fmin(a, b) : (k < NMIN + NMAX ? fmax(a, b) : a + b);
}
template <int NMIN, int NMAX>
__device__ __forceinline__ double stat_wave(int k, double v) {
    return k < NMIN ? wave_min(v) : (k < NMIN + NMAX ? wave_max(v) : wave_sum(v));
}

// the tail of a statistics kernel of B threads: joins every thread's v over the block into partial[blockIdx.x * N + k]
template <int NMIN, int NMAX, int B, int N>
__device__ __forceinline__ void stats_block_partial(const double (&v)[N], double *__restrict__ partial) {
    __shared__ double sm[N][B / WAVE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double r = stat_wave<NMIN, NMAX>(k, v[k]);
        if (lane == 0) sm[k][wv] = r;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        double r = sm[k][0];
        for (int w = 1; w < B / WAVE; w++) r = stat_join<NMIN, NMAX>(k, r, sm[k][w]);
        partial[(int64_t)blockIdx.x * N + k] = r;
    }
}

// joins the nblocks rows of partial: one wave per statistic
template <int N, int NMIN, int NMAX>
__global__ __launch_bounds__(N * WAVE) void stats_final(const double *__restrict__ partial, int nblocks,
                                                        double *__restrict__ out) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double r = stat_identity<NMIN, NMAX>(k);
    for (int b = lane; b < nblocks; b += 64) r = stat_join<NMIN, NMAX>(k, r, partial[b * N + k]);
    r = stat_wave<NMIN, NMAX>(k, r);
    if (lane == 0) out[k] = r;
}

constexpr int PIECE = 16 * WAVE;   // positions per piece: 16 per lane

// Segment s (a bin, a group) of the sorted sequence is [start[s], start[s + 1]).  Its pieces sit at the piece slots from
// piece_base(start, s) on: injective in (segment, piece), and at most n / PIECE + n_seg + 1 slots for n positions.
__device__ __forceinline__ int64_t piece_base(const int32_t *start, int64_t s) { return start[s] / PIECE + s; }

// Piece slot g of n_seg >= 1 segments -> the segment and the sorted positions [p0, p1) of the piece; false for the slots
// that no (segment, piece) maps to.
__device__ __forceinline__ bool piece_locate(const int32_t *start, int64_t n_seg, int64_t g, int64_t &seg, int64_t &p0,
                                             int64_t &p1) {
    int64_t lo = 0, hi = n_seg - 1;                     // the last segment whose base is <= g
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (piece_base(start, mid) <= g) lo = mid; else hi = mid - 1;
    }
    const int64_t k = g - piece_base(start, lo);
    const int64_t first = (int64_t)start[lo] + k * PIECE, end = start[lo + 1];
    if (k < 0 || first >= end) return false;
    seg = lo;
    p0 = first;
    p1 = min(end, first + PIECE);
    return true;
}

}  // namespace sph
