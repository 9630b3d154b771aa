// exact_sum.hpp -- the exact sums of pair_stats.hip (sph_pairs), history.hip (sph_history), modes.hip (sph_modes) and
// frames.hip (sph_frames): a term is formed in double, scaled by a power of two that a bound on the terms fixes, rounded
// half-even to a 64-bit integer and added into a 128-bit integer {lo, hi}; the total is converted to a double once.  Integer
// addition is associative, so a sum does not depend on the order, the launch or the shape of its reduction.  The arithmetic
// and the shapes built on it -- the contended add, the block's LDS histogram of limbs, the slab sum, the conversions --
// live here (DESIGN sections 26, 27, 29, 30 and 31).
#pragma once
#include <cmath>
#include <cstdint>

#include "sph_internal.hpp"

namespace sph {

__device__ __forceinline__ bool finite(double a) { return fabs(a) <= 1.7976931348623157e308; }

// the exponent e with b < 2^e (b >= 0 and finite; 0 for b = 0)
__device__ __forceinline__ int32_t exp_above(double b) {
    int e = 0;
    (void)frexp(b, &e);
    return (int32_t)e;
}

// term 2^sh rounded half-even to an integer (|.| <= 2^62 by the bound that fixed sh)
__device__ __forceinline__ long long to_fixed(double term, int sh) { return (long long)rint(ldexp(term, sh)); }

// {lo, hi} += the sign-extended 64-bit t
__device__ __forceinline__ void add_fixed(unsigned long long &lo, unsigned long long &hi, long long t) {
    const unsigned long long tu = (unsigned long long)t;
    lo += tu;
    hi += (unsigned long long)(t >> 63) + (unsigned long long)(lo < tu);
}

// {lo, hi} += {l, h}
__device__ __forceinline__ void add_limbs(unsigned long long &lo, unsigned long long &hi, unsigned long long l,
                                          unsigned long long h) {
    lo += l;
    hi += h + (unsigned long long)(lo < l);
}

// {*lo, *hi} += {l, h} where other lanes add to the accumulator as well (LDS or global): the low word with a returning add,
// the high word gets h plus the carry the returned value shows, and no add where that is zero
__device__ __forceinline__ void add_limbs_shared(unsigned long long *lo, unsigned long long *hi, unsigned long long l,
                                                 unsigned long long h) {
    const unsigned long long old = atomicAdd(lo, l);
    const unsigned long long up = h + (unsigned long long)(old + l < old);
    if (up != 0ull) atomicAdd(hi, up);
}

// term 2^sh, rounded half-even to an integer, added into the shared accumulator {h[0], h[1]} (an LDS histogram)
__device__ __forceinline__ void add_term(unsigned long long *h, double term, int sh) {
    const long long t = to_fixed(term, sh);
    add_limbs_shared(h, h + 1, (unsigned long long)t, (unsigned long long)(t >> 63));
}

// the sum of {lo, hi} over the 64 lanes (xor butterfly of 128-bit additions): every lane ends with the same result
__device__ __forceinline__ void wave_add_limbs(unsigned long long &lo, unsigned long long &hi) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long l = __shfl_xor(lo, o, 64), h = __shfl_xor(hi, o, 64);
        add_limbs(lo, hi, l, h);
    }
}

// The LDS histogram of a block of nt threads (pairs_bin, modes_rings): `acc` accumulators {lo, hi} in `copies` copies, copy c
// at hist + 2 c acc, dealt by lane so that fewer lanes add to the same address.  The kernel declares hist[2 * HIST], loops
// over its chunks and sets the barriers: before hist_zero (the last flush is done), after it, and before hist_flush.
// (copies comes before acc in the three signatures on purpose: the kernels' scalar registers)
constexpr int HIST = 3072;                 // accumulators of a block's histogram (48 KB), all copies together
constexpr int MAX_COPIES = 8;
constexpr size_t SLAB_BYTES = (size_t)64 << 20;   // the budget of a pass's slabs, one per block
__device__ __forceinline__ void hist_zero(unsigned long long *hist, int copies, int acc, int nt) {
    for (int k = threadIdx.x; k < 2 * copies * acc; k += nt) hist[k] = 0ull;
}
__device__ __forceinline__ unsigned long long *hist_mine(unsigned long long *hist, int copies, int acc) {
    return hist + 2 * (threadIdx.x % copies) * acc;
}
// out[2 k], out[2 k + 1] = accumulator k added over the copies, plain stores
__device__ __forceinline__ void hist_flush(const unsigned long long *hist, int copies, int acc, int nt, unsigned long long *out) {
    for (int k = threadIdx.x; k < acc; k += nt) {
        unsigned long long lo = 0, up = 0;
        for (int c = 0; c < copies; c++) add_limbs(lo, up, hist[2 * (c * acc + k)], hist[2 * (c * acc + k) + 1]);
        out[2 * k] = lo;
        out[2 * k + 1] = up;
    }
}

// The histogram's sizing on the host, for `segs` segments (bins, rings) of `na` accumulators each: the segments a block
// holds at a time, the copies of them, and the slabs (blocks) of the pass, at most max_blocks and within SLAB_BYTES.
// MAX_NA: the descriptor's largest na (sph_pairs: nsum <= 14, sph_modes: na <= 19), so one segment always fits: chunk >= 1.
struct HistPlan { int chunk, copies, nslab; };
template <int MAX_NA>
inline HistPlan hist_plan(int segs, int na, int64_t max_blocks) {
    static_assert(MAX_NA >= 1 && MAX_NA <= HIST, "a segment's accumulators must fit the histogram");
    HistPlan p;
    p.chunk = std::min(segs, HIST / na);
    p.copies = std::max(1, std::min(MAX_COPIES, HIST / (p.chunk * na)));
    p.nslab = (int)std::max<int64_t>(1, std::min<int64_t>(max_blocks, (int64_t)(SLAB_BYTES / ((size_t)segs * (size_t)na * 16))));
    return p;
}

// {lo, hi} = accumulator g added over nslab slabs of n_acc accumulators each, by one wavefront: lane l adds the slabs l,
// l + 64, ..., then the butterfly
__device__ __forceinline__ void slab_sum(const unsigned long long *__restrict__ slab, int nslab, int64_t n_acc, int64_t g, int lane,
                                         unsigned long long &lo, unsigned long long &hi) {
    lo = hi = 0ull;
    for (int b = lane; b < nslab; b += WAVE) add_limbs(lo, hi, slab[2 * ((size_t)b * n_acc + g)], slab[2 * ((size_t)b * n_acc + g) + 1]);
    wave_add_limbs(lo, hi);
}

// {lo, hi} 2^(e - 62), correctly rounded: the magnitude normalised to its top 64 bits with the rest as a sticky bit (the
// bits below a double's rounding position), then u64 -> f64 rounds half-even once, then an exact scaling
__device__ __forceinline__ double limbs_to_double(unsigned long long lo, unsigned long long hi, int e) {
    const bool neg = (long long)hi < 0;
    if (neg) {
        lo = ~lo + 1ull;
        hi = ~hi + (lo == 0ull);
    }
    if ((lo | hi) == 0ull) return 0.0;
    const int lz = hi ? __clzll((long long)hi) : 64 + __clzll((long long)lo);
    unsigned long long top, rest;
    if (lz >= 64) {
        top = lo << (lz - 64);
        rest = 0ull;
    } else if (lz == 0) {
        top = hi;
        rest = lo;
    } else {
        top = (hi << lz) | (lo >> (64 - lz));
        rest = lo << lz;
    }
    if (rest) top |= 1ull;
    const double d = ldexp((double)top, 64 - lz + e - 62);
    return neg ? -d : d;
}

// the same conversion on the host
inline double finish_one(uint64_t lo, uint64_t hi, int e) {
    const __int128 v = (__int128)(((unsigned __int128)hi << 64) | (unsigned __int128)lo);
    return std::ldexp((double)v, e - 62);                // int128 -> double rounds half-even once; the scaling is exact
}
// sums[g] = raw[g] 2^(exps[g % nsum] - 62), g in [0, n_acc)
inline void finish_all(const uint64_t *raw, int64_t n_acc, const int32_t *exps, int nsum, double *sums) {
    for (int64_t g = 0; g < n_acc; g++) sums[g] = finish_one(raw[2 * g], raw[2 * g + 1], exps[g % nsum]);
}

}  // namespace sph
