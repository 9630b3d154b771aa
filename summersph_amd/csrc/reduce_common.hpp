// reduce_common.hpp -- the wavefront reductions and the "piece" shape of the order-free sums (profile.hip, energy.hip,
// groups.hip): a run of sorted positions is cut into pieces of PIECE positions from its own start, one wavefront reduces
// each piece (lane l adds positions l, l + 64, ... in turn, then the butterfly) and a second kernel adds a run's pieces in
// the same shape.  A sum's shape then depends on its run's start and length alone, never on the launch.
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
